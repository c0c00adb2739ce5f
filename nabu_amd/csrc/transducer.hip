// transducer.hip — RNN transducer (Graves 2012) with the additive joint h[t,u,k] = f[t,k] + g[u,k]: loss and gradients
// over the T x (U+1) lattice, and one step of the greedy search.  Contract: include/nabu_hip.h,
// nabu_transducer_loss_grad and nabu_transducer_greedy_step.
//
// Three launches, none of which materialises h [B,T,U1,C]:
//   (a) emission terms   a thread per node (t,u): maximum and log-sum of h[t,u,:] (each node takes its own maximum
//                        before exp), lb = log p(blank), ly = log p(labels[u]);
//   (b) sweeps           alpha and beta side by side (blockIdx.y), an utterance per blockIdx.x, walking anti-diagonals
//                        d = t + u.  Two routes with ONE per-node expression, so their results are the same bits:
//                          wave       U1 <= 64: one wave64 per sweep, lane u holds node (d-u, u); the neighbour comes
//                                     through a DPP wave shift, no barrier in the loop, lb / ly loaded 8 .. 16
//                                     diagonals ahead;
//                          workgroup  256 threads, u strided, the previous diagonal in LDS, one barrier per diagonal;
//   (c) gradients        a workgroup per df row (b,t) and per dg row (b,u): the occupations of the row's nodes are
//                        worked out once into LDS, then G[t,u,k] is recomputed and summed along the row in a fixed
//                        order (node j goes to part j mod P, the parts are added in part order).
// The workspace holds the per-node arrays SKEWED: node (t,u) sits at row d = t + u, column u, so a diagonal is
// contiguous: the sweeps' loads and stores are coalesced and their addresses known ahead.
#include <stdlib.h>

#include "transducer_dev.h"

namespace nabu {

struct TransArgs {
  int B, T, U1, C, ldl;
  const float *f, *g;
  const int32_t *enc_len, *labels, *label_len;
  float grad_scale;
  float *nll, *df, *dg;
  int32_t *status;
  // workspace: six skewed arrays [B][T+U1][U1], then the utterances' verdicts
  float *mx, *lz, *lb, *ly, *al, *be;
  int32_t *bad;
};

__device__ __forceinline__ size_t tr_slab(const TransArgs &p, int b) { return (size_t)b * (p.T + p.U1) * p.U1; }

__device__ __forceinline__ float tr_dn(float v, float fill) {     // lane i <- lane i+1 (lane 63 <- fill)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
// two-term log-sum-exp on the hardware exp2 / log2: it sits on the diagonal-to-diagonal chain.  The argument of exp is
// <= 0 and that of log in [1, 2]: the scaling's relative error |x| 2^-24 is an absolute one below 2^-24 in the result
__device__ __forceinline__ float tr_lse2(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  return m + __logf(1.0f + __expf(n - m));
}
// the node expressions of both routes
__device__ __forceinline__ float tr_alpha_node(float a_stay, float lb_stay, float emit) { return tr_lse2(a_stay + lb_stay, emit); }
__device__ __forceinline__ float tr_beta_node(float b_stay, float b_emit, float lb, float ly) {
  return tr_lse2(b_stay + lb, b_emit + ly);
}

// ---------------------------------------------------------------------------------------------------------------
// (a) grid (ceil(T U1 / 256), B).  Lengths are clamped and labels guarded here: the verdict on an utterance is (b)'s
__global__ __launch_bounds__(TR_NT) void transducer_emit_kernel(TransArgs p) {
  const int b = blockIdx.y, C = p.C, blank = p.C - 1;
  const int idx = blockIdx.x * TR_NT + threadIdx.x;
  if (idx >= p.T * p.U1) return;
  const int t = idx / p.U1, u = idx - t * p.U1;
  const int Tb = tr_clamp(p.enc_len[b], 0, p.T), Ub = tr_clamp(p.label_len[b], 0, p.U1 - 1);
  if (t >= Tb || u > Ub) return;
  const float *fr = p.f + ((size_t)b * p.T + t) * C, *gr = p.g + ((size_t)b * p.U1 + u) * C;
  int lab = u < Ub ? p.labels[(size_t)b * p.ldl + u] : -1;
  if (lab >= blank) lab = -1;
  const size_t at = tr_slab(p, b) + (size_t)(t + u) * p.U1 + u;
  tr_node_terms(fr, gr, C, lab, p.mx + at, p.lz + at, p.lb + at, p.ly + at);     // (transducer_dev.h)
}

// ---------------------------------------------------------------------------------------------------------------
// (b) the verdict on utterance b, the same in every thread of the workgroup (one barrier)
__device__ bool tr_utt_bad(const TransArgs &p, int b, int tid, int nt) {
  return tr_lengths_labels_bad(p.T, p.U1, p.C, p.enc_len, p.labels, p.ldl, p.label_len, b, tid, nt);
}

// a rejected utterance: nll 0, its verdict for (c), and its number in the status word (the beta workgroup's thread 0)
__device__ void tr_reject(const TransArgs &p, int b) {
  p.nll[b] = 0.f;
  p.bad[b] = 1;
  tr_status_first(p.status, b);
}

// wave route: grid (B, 2), 64 threads.  blockIdx.y: 0 alpha, 1 beta
__global__ __launch_bounds__(64) void transducer_sweep_wave_kernel(TransArgs p) {
  const int b = blockIdx.x, lane = threadIdx.x, U1 = p.U1;
  const bool beta = blockIdx.y == 1;
  if (tr_utt_bad(p, b, lane, 64)) {
    if (beta && lane == 0) tr_reject(p, b);
    return;
  }
  const int Tb = p.enc_len[b], Ub = p.label_len[b], D = Tb + Ub;       // diagonals 0 .. D-1
  const size_t slab = tr_slab(p, b);
  const int lu = lane < U1 ? lane : U1 - 1;            // (a column inside the row for the idle lanes' loads)
  const float *lbp = p.lb + slab + lu, *lyp = p.ly + slab + lu;
  const bool mine = lane <= Ub;
  if (!beta) {
    // diagonal d is made from the terms of diagonal d-1: node (t-1,u) stays in its lane, node (t,u-1) hands its
    // alpha + ly one lane up
    float *out = p.al + slab + lu;
    float a = lane == 0 ? 0.f : TR_NEG;
    if (lane == 0) out[0] = a;
    float nb[TR_AHEAD], ny[TR_AHEAD];
#pragma unroll
    for (int j = 0; j < TR_AHEAD; ++j) {
      const int dd = j < D ? j : D - 1;
      nb[j] = lbp[(size_t)dd * U1];
      ny[j] = lyp[(size_t)dd * U1];
    }
    for (int d0 = 1; d0 < D; d0 += TR_AHEAD) {
      float cb[TR_AHEAD], cy[TR_AHEAD];
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        cb[j] = nb[j];
        cy[j] = ny[j];
      }
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        int dd = d0 - 1 + TR_AHEAD + j;
        dd = dd < D ? dd : D - 1;
        nb[j] = lbp[(size_t)dd * U1];
        ny[j] = lyp[(size_t)dd * U1];
      }
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        const int d = d0 + j;
        if (d < D) {
          const int t = d - lane;
          const bool from = mine && t >= 1 && t <= Tb;          // node (t-1, u) exists: its terms are written
          const float emit = tr_up(a + (from ? cy[j] : TR_NEG), TR_NEG);
          const float n = tr_alpha_node(a, from ? cb[j] : TR_NEG, emit);
          const bool here = mine && t >= 0 && t < Tb;
          a = here ? n : TR_NEG;
          if (here) out[(size_t)d * U1] = a;
        }
      }
    }
  } else {
    // diagonal d is made from diagonal d+1 and its OWN terms: node (t+1,u) stays in its lane, node (t,u+1) comes one
    // lane down.  The virtual node (Tb, Ub) = 0 behind the final blank starts it
    float *out = p.be + slab + lu;
    float v = lane == Ub ? 0.f : TR_NEG;
    float nb[TR_AHEAD], ny[TR_AHEAD];
#pragma unroll
    for (int j = 0; j < TR_AHEAD; ++j) {
      const int dd = D - 1 - j >= 0 ? D - 1 - j : 0;
      nb[j] = lbp[(size_t)dd * U1];
      ny[j] = lyp[(size_t)dd * U1];
    }
    for (int d0 = D - 1; d0 >= 0; d0 -= TR_AHEAD) {
      float cb[TR_AHEAD], cy[TR_AHEAD];
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        cb[j] = nb[j];
        cy[j] = ny[j];
      }
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        int dd = d0 - TR_AHEAD - j;
        dd = dd >= 0 ? dd : 0;
        nb[j] = lbp[(size_t)dd * U1];
        ny[j] = lyp[(size_t)dd * U1];
      }
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        const int d = d0 - j;
        if (d >= 0) {
          const int t = d - lane;
          const bool here = mine && t >= 0 && t < Tb;
          const float dn = tr_dn(v, TR_NEG);
          const float n = tr_beta_node(v, dn, here ? cb[j] : TR_NEG, here ? cy[j] : TR_NEG);
          v = here ? n : TR_NEG;
          if (here) out[(size_t)d * U1] = v;
        }
      }
    }
    if (lane == 0) {
      p.nll[b] = -v;            // node (0,0)
      p.bad[b] = 0;
    }
  }
}

// workgroup route: grid (B, 2), 256 threads, LDS: two rows of U1 floats (the previous diagonal and the one being made)
__global__ __launch_bounds__(TR_NT) void transducer_sweep_wg_kernel(TransArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x, U1 = p.U1;
  const bool beta = blockIdx.y == 1;
  if (tr_utt_bad(p, b, tid, TR_NT)) {
    if (beta && tid == 0) tr_reject(p, b);
    return;
  }
  const int Tb = p.enc_len[b], Ub = p.label_len[b], D = Tb + Ub;
  const size_t slab = tr_slab(p, b);
  const float *lbp = p.lb + slab, *lyp = p.ly + slab;
  float *prev = smem, *cur = smem + U1;
  if (!beta) {
    float *out = p.al + slab;
    for (int u = tid; u <= Ub; u += TR_NT) prev[u] = u == 0 ? 0.f : TR_NEG;
    if (tid == 0) out[0] = 0.f;
    __syncthreads();
    for (int d = 1; d < D; ++d) {
      for (int u = tid; u <= Ub; u += TR_NT) {
        const int t = d - u;
        const bool from = t >= 1 && t <= Tb;
        float emit = TR_NEG;                                     // (the fill of the wave route's shift)
        if (u >= 1) {
          const bool lfrom = t >= 0 && t < Tb;                   // node (t, u-1) exists
          emit = prev[u - 1] + (lfrom ? lyp[(size_t)(d - 1) * U1 + u - 1] : TR_NEG);
        }
        const float n = tr_alpha_node(prev[u], from ? lbp[(size_t)(d - 1) * U1 + u] : TR_NEG, emit);
        const bool here = t >= 0 && t < Tb;
        const float a = here ? n : TR_NEG;
        cur[u] = a;
        if (here) out[(size_t)d * U1 + u] = a;
      }
      __syncthreads();
      float *tmp = prev; prev = cur; cur = tmp;
    }
  } else {
    float *out = p.be + slab;
    for (int u = tid; u <= Ub; u += TR_NT) prev[u] = u == Ub ? 0.f : TR_NEG;
    __syncthreads();
    for (int d = D - 1; d >= 0; --d) {
      for (int u = tid; u <= Ub; u += TR_NT) {
        const int t = d - u;
        const bool here = t >= 0 && t < Tb;
        const float dn = u < Ub ? prev[u + 1] : TR_NEG;
        const float n = tr_beta_node(prev[u], dn, here ? lbp[(size_t)d * U1 + u] : TR_NEG,
                                     here ? lyp[(size_t)d * U1 + u] : TR_NEG);
        const float v = here ? n : TR_NEG;
        cur[u] = v;
        if (here) out[(size_t)d * U1 + u] = v;
      }
      __syncthreads();
      float *tmp = prev; prev = cur; cur = tmp;
    }
    if (tid == 0) {
      p.nll[b] = -prev[0];
      p.bad[b] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// (c) grid B T + B U1, 256 threads.  Workgroup r < B T: row (b,t) of df, the sum over u; the others: row (b,u) of dg,
// the sum over t.  Per group of 256 nodes of the row: a thread per node works out
//   occ = exp(alpha + beta + nll), tb = exp(alpha + lb + beta[t+1,u] + nll), ty = exp(alpha + ly + beta[t,u+1] + nll)
// into LDS; then thread (part, k) adds G = occ p(k) - [k = blank] tb - [k = label] ty of the nodes j = part, part + P, ..
// of the group.  The parts are added in part order at the end: one fixed order, no atomics.
__global__ __launch_bounds__(TR_NT) void transducer_grad_kernel(TransArgs p) {
  __shared__ float s_occ[TR_NT], s_tb[TR_NT], s_ty[TR_NT], s_mx[TR_NT], s_lz[TR_NT], s_red[TR_NT];
  __shared__ int s_lab[TR_NT];
  const int tid = threadIdx.x, C = p.C, U1 = p.U1, T = p.T, blank = p.C - 1;
  const bool is_df = (int)blockIdx.x < p.B * T;
  const int r = is_df ? blockIdx.x : blockIdx.x - p.B * T;
  const int b = is_df ? r / T : r / U1, row = is_df ? r - b * T : r - b * U1;
  float *dst = is_df ? p.df + ((size_t)b * T + row) * C : p.dg + ((size_t)b * U1 + row) * C;
  const bool bad = p.bad[b] != 0;
  const int Tb = bad ? 0 : p.enc_len[b], Ub = bad ? -1 : p.label_len[b];
  const int n = is_df ? Ub + 1 : Tb;                     // nodes of the row
  if (bad || (is_df ? row >= Tb : row > Ub)) {
    for (int k = tid; k < C; k += TR_NT) dst[k] = 0.f;
    return;
  }
  const size_t slab = tr_slab(p, b);
  const float nll = p.nll[b];
  const float *fix = is_df ? p.f + ((size_t)b * T + row) * C : p.g + ((size_t)b * U1 + row) * C;   // the row's own logits
  const float *var = is_df ? p.g + (size_t)b * U1 * C : p.f + (size_t)b * T * C;                  // the other side's
  for (int k0 = 0; k0 < C; k0 += TR_NT) {
    const int kc = C - k0 < TR_NT ? C - k0 : TR_NT, P = TR_NT / kc;
    const int part = tid / kc, k = k0 + tid - part * kc;
    const bool act = part < P;
    const float xk = act ? fix[k] : 0.f;
    float acc = 0.f;
    for (int j0 = 0; j0 < n; j0 += TR_NT) {
      const int j = j0 + tid;
      if (j < n) {
        const int t = is_df ? row : j, u = is_df ? j : row;
        const size_t at = slab + (size_t)(t + u) * U1 + u;
        const float a = p.al[at], lbn = p.lb[at], lyn = p.ly[at];
        const float bt = t + 1 < Tb ? p.be[at + U1] : (u == Ub ? 0.f : TR_NEG);     // beta[Tb, Ub] reads as 0
        const float bu = u < Ub ? p.be[at + U1 + 1] : TR_NEG;
        s_occ[tid] = expf((a + p.be[at]) + nll);
        s_tb[tid] = expf(((a + lbn) + bt) + nll);
        s_ty[tid] = expf(((a + lyn) + bu) + nll);
        s_mx[tid] = p.mx[at];
        s_lz[tid] = p.lz[at];
        s_lab[tid] = u < Ub ? p.labels[(size_t)b * p.ldl + u] : -1;
      }
      __syncthreads();
      if (act) {
        const int m = n - j0 < TR_NT ? n - j0 : TR_NT;
        for (int i = part; i < m; i += P) {
          const float h = xk + var[(size_t)(j0 + i) * C + k];
          float gk = s_occ[i] * __expf((h - s_mx[i]) - s_lz[i]);
          if (k == blank) gk -= s_tb[i];
          if (k == s_lab[i]) gk -= s_ty[i];
          acc += gk;
        }
      }
      __syncthreads();
    }
    s_red[tid] = acc;
    __syncthreads();
    if (tid < kc) {
      float tot = s_red[tid];
      for (int q = 1; q < P; ++q) tot += s_red[q * kc + tid];
      dst[k] = p.grad_scale * tot;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// one step of the greedy search: grid B, one wave per row
__global__ __launch_bounds__(64) void transducer_greedy_kernel(int T, int C, int S, int step, const float *f,
                                                               const float *g_row, const int32_t *enc_len, int32_t *t_pos,
                                                               int32_t *out_len, int32_t *ids, int32_t *emit,
                                                               int32_t *last_id, float *score) {
  const int b = blockIdx.x, lane = threadIdx.x, blank = C - 1;
  int tp, ol;
  float sc;
  if (step == 0) {                 // the first step of a search sets the row's state up
    tp = 0; ol = 0; sc = 0.f;
    for (int i = lane; i < S; i += 64) ids[(size_t)b * S + i] = -1;
    if (lane == 0) last_id[b] = blank;
  } else {
    tp = t_pos[b]; ol = out_len[b]; sc = score[b];
  }
  const int el = enc_len[b] < T ? enc_len[b] : T;
  if (tp >= el || ol >= S) {
    if (lane == 0) {
      emit[b] = 0;
      if (step == 0) { t_pos[b] = tp; out_len[b] = ol; score[b] = sc; }
    }
    return;
  }
  const float *fr = f + ((size_t)b * T + tp) * C, *gr = g_row + (size_t)b * C;
  float best = -__builtin_inff();
  int arg = 0x7fffffff;
  for (int k = lane; k < C; k += 64) {
    const float v = fr[k] + gr[k];
    if (v > best || arg == 0x7fffffff) { best = v; arg = k; }      // strictly greater: the smallest index of a lane stays
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
  }
  float z = 0.f;
  for (int k = lane; k < C; k += 64) z += expf((fr[k] + gr[k]) - best);
  z = wave_sum(z);
  if (lane == 0) {
    score[b] = sc + (0.f - logf(z));                 // (x - max) - log sum exp, and x is the maximum
    if (arg == blank) {
      t_pos[b] = tp + 1;
      out_len[b] = ol;
      emit[b] = 0;
    } else {
      ids[(size_t)b * S + ol] = arg;
      t_pos[b] = tp;
      out_len[b] = ol + 1;
      last_id[b] = arg;
      emit[b] = 1;
    }
  }
}

static size_t trans_nodes(int B, int T, int U1) { return (size_t)B * ((size_t)T + U1) * U1; }

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_transducer_ws_bytes(int B, int T, int U1) {
  if (B <= 0 || T <= 0 || U1 <= 0) return 0;
  return 6 * align_up(trans_nodes(B, T, U1) * sizeof(float), 16) + align_up((size_t)B * sizeof(int32_t), 16);
}

extern "C" int nabu_transducer_loss_grad(int B, int T, int U1, int C, const float *f, const float *g,
                                         const int32_t *enc_len, const int32_t *labels, int ldl,
                                         const int32_t *label_len, float grad_scale, float *nll, float *df, float *dg,
                                         int32_t *status, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && U1 > 0 && C > 1, "transducer_loss_grad: bad dimensions");
  NABU_CHECK_ARG(f && g && enc_len && label_len && nll && df && dg && status && ws, "transducer_loss_grad: null pointer");
  NABU_CHECK_ARG(U1 == 1 || (labels && ldl >= U1 - 1), "transducer_loss_grad: null labels or ldl < U1 - 1");
  NABU_CHECK_ARG((size_t)T * U1 < ((size_t)1 << 31) && (size_t)B * ((size_t)T + U1) < ((size_t)1 << 31),
                 "transducer_loss_grad: T * U1 or B * (T + U1) does not fit an int");
  const size_t need = nabu_transducer_ws_bytes(B, T, U1);
  if (ws_bytes < need) return fail(NABU_EWS, "transducer_loss_grad: workspace %zu < %zu", ws_bytes, need);
  static const int force_wg = env_int("NABU_TRANSDUCER_WORKGROUP", 0);   // 1: the workgroup route for every shape (A/B tests)
  const bool wave = !force_wg && U1 <= 64;
  const size_t shm = 2 * (size_t)U1 * sizeof(float);
  if (!wave && shm > 150 * 1024)
    return fail(NABU_EUNSUP, "transducer_loss_grad: U1=%d needs %zu B of LDS", U1, shm);
  hipStream_t s = static_cast<hipStream_t>(stream);
  TransArgs p;
  p.B = B; p.T = T; p.U1 = U1; p.C = C; p.ldl = ldl;
  p.f = f; p.g = g; p.enc_len = enc_len; p.labels = labels; p.label_len = label_len;
  p.grad_scale = grad_scale; p.nll = nll; p.df = df; p.dg = dg; p.status = status;
  const size_t arr = align_up(trans_nodes(B, T, U1) * sizeof(float), 16) / sizeof(float);
  float *w = static_cast<float *>(ws);
  p.mx = w; p.lz = w + arr; p.lb = w + 2 * arr; p.ly = w + 3 * arr; p.al = w + 4 * arr; p.be = w + 5 * arr;
  p.bad = reinterpret_cast<int32_t *>(w + 6 * arr);
  // measurement only (tools/transducer_bench.py): a mask of the launches to make — 1 emission terms, 2 sweeps,
  // 4 gradients — on a workspace that a complete call with the same operands has filled.  Read on every call
  const int todo = env_int("NABU_TRANSDUCER_LAUNCHES", 7);
  NABU_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  const int nodes = T * U1;
  if (todo & 1) {
    hipLaunchKernelGGL(transducer_emit_kernel, dim3((nodes + TR_NT - 1) / TR_NT, B), dim3(TR_NT), 0, s, p);
    NABU_LAUNCH_CHECK();
  }
  if ((todo & 2) && wave) {
    hipLaunchKernelGGL(transducer_sweep_wave_kernel, dim3(B, 2), dim3(64), 0, s, p);
    NABU_LAUNCH_CHECK();
  } else if (todo & 2) {
    NABU_TRY(launch_lds(transducer_sweep_wg_kernel, dim3(B, 2), dim3(TR_NT), shm, s, p));
  }
  if (todo & 4) {
    hipLaunchKernelGGL(transducer_grad_kernel, dim3(B * (T + U1)), dim3(TR_NT), 0, s, p);
    NABU_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int nabu_transducer_greedy_step(int B, int T, int C, int S, int step, const float *f, const float *g_row,
                                           const int32_t *enc_len, int32_t *t_pos, int32_t *out_len, int32_t *ids,
                                           int32_t *emit, int32_t *last_id, float *score, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && C > 1 && S > 0 && step >= 0, "transducer_greedy_step: bad dimensions");
  NABU_CHECK_ARG(f && g_row && enc_len && t_pos && out_len && ids && emit && last_id && score,
                 "transducer_greedy_step: null pointer");
  hipLaunchKernelGGL(transducer_greedy_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), T, C, S, step, f,
                     g_row, enc_len, t_pos, out_len, ids, emit, last_id, score);
  NABU_LAUNCH_CHECK();
  return 0;
}
