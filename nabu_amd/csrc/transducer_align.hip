// transducer_align.hip — forced alignment with a transducer model: the best monotone path through the T x (U+1)
// lattice the loss sums over (transducer.hip), the frame of every label, its log-probability and the path's score.
// Contract: include/nabu_hip.h, nabu_transducer_align.
//
// The frame normalisers depend on the node (t,u), so — unlike ctc_align.hip — the recursion runs on log-probabilities:
// the loss's lb and ly, made by the loss's own node expression (tr_node_terms, transducer_dev.h) into the loss's skewed
// layout (node (t,u) at row d = t + u, column u).  Two launches:
//   (a) emission terms   a thread per node: lb and ly only (the loss's other four arrays are not needed);
//   (b) sweep, backtrace and outputs, a workgroup of 256 per utterance.  The max-plus sweep walks anti-diagonals like
//       the loss's alpha sweep, on two routes with ONE per-node expression (tra_node):
//         wave       U1 <= 64: wave 0 alone, lane u on node (d-u, u), the neighbour through a DPP wave shift, no
//                    barrier in the loop, lb / ly loaded 8 .. 16 diagonals ahead;
//         workgroup  256 threads, u strided, the previous diagonal in LDS, one barrier per diagonal.
//       ONE bit per node says which move made it, and the comparison's own lane mask is that bit for 64 nodes: the
//       back-pointers of diagonal d and columns 64c .. 64c+63 are one 64-bit word, bp[d * W + c] (W = ceil(U1 / 64)).
//       The backtrace steps one diagonal back per move, so its addresses do not depend on the path: wave 0 loads the
//       words of 64 diagonals in one go (lane j that of diagonal d-j) and walks them with v_readlane and scalar
//       arithmetic, no memory access on the chain; a word column ends the run early (workgroup route only).  The path
//       (u per diagonal) leaves as one store per run.  Then all 256 threads turn the path into state / frame / conf and
//       sum the score in a fixed order.
// Back-pointers and path live in LDS while they fit, in the caller's workspace otherwise.
#include <stdlib.h>

#include "transducer_dev.h"

namespace nabu {

struct TrAlignArgs {
  int B, T, U1, C, ldl, W;              // W: 64-bit back-pointer words per diagonal
  const float *f, *g;
  const int32_t *enc_len, *labels, *label_len;
  int32_t *state, *frame;
  float *conf, *score;
  int32_t *status;
  float *lb, *ly;                       // workspace: two skewed arrays [B][T+U1][U1]
  unsigned char *trace_ws;              // workspace back-pointers and path, trace_stride bytes per utterance
  size_t trace_stride;
};

__device__ __forceinline__ size_t tra_slab(const TrAlignArgs &p, int b) { return (size_t)b * (p.T + p.U1) * p.U1; }

// the node expression of both routes: stay = v[t-1,u] + lb[t-1,u], emit = v[t,u-1] + ly[t,u-1], each one float32
// addition made by the caller.  A tie keeps the blank move.  The bit says what the comparison found; which moves EXIST
// is the backtrace's business (tra_backtrace)
__device__ __forceinline__ float tra_node(float stay, float emit, bool *label_move) {
  *label_move = emit > stay;
  return *label_move ? emit : stay;
}

// ---------------------------------------------------------------------------------------------------------------
// (a) grid (ceil(T U1 / 256), B): transducer_emit_kernel's nodes and guards, lb and ly only
__global__ __launch_bounds__(TR_NT) void transducer_align_emit_kernel(TrAlignArgs p) {
  const int b = blockIdx.y, C = p.C, blank = p.C - 1;
  const int idx = blockIdx.x * TR_NT + threadIdx.x;
  if (idx >= p.T * p.U1) return;
  const int t = idx / p.U1, u = idx - t * p.U1;
  const int Tb = tr_clamp(p.enc_len[b], 0, p.T), Ub = tr_clamp(p.label_len[b], 0, p.U1 - 1);
  if (t >= Tb || u > Ub) return;
  const float *fr = p.f + ((size_t)b * p.T + t) * C, *gr = p.g + ((size_t)b * p.U1 + u) * C;
  int lab = u < Ub ? p.labels[(size_t)b * p.ldl + u] : -1;
  if (lab >= blank) lab = -1;
  const size_t at = tra_slab(p, b) + (size_t)(t + u) * p.U1 + u;
  float m, l;
  tr_node_terms(fr, gr, C, lab, &m, &l, p.lb + at, p.ly + at);
}

// ---------------------------------------------------------------------------------------------------------------
// a rejected utterance: score -inf, state / frame -1, conf 0, and its number in the status word
__device__ void tra_reject(const TrAlignArgs &p, int b, int tid) {
  for (int t = tid; t < p.T; t += TR_NT) p.state[(size_t)b * p.T + t] = -1;
  for (int i = tid; i < p.U1 - 1; i += TR_NT) {
    p.frame[(size_t)b * (p.U1 - 1) + i] = -1;
    p.conf[(size_t)b * (p.U1 - 1) + i] = 0.f;
  }
  if (tid == 0) {
    p.score[b] = -__builtin_inff();
    tr_status_first(p.status, b);
  }
}

// Wave 0, behind the sweep: from the final blank's node (Tb-1, Ub) on diagonal D-1 back to (0,0).  path[d] = the u of
// the path's node on diagonal d.  u and d are the same in every lane: the chain is scalar shifts and subtractions.
// A node takes the label move if its bit says so, among the moves that EXIST: column 0 has no label move and frame 0
// (u = d) no blank move, whatever the bit says.  With finite terms the bits say the same (a missing move is the finite
// -1e30 and loses); with -inf or NaN terms (a masked blank, a diverged model: v + lb falls below -1e30) they need not,
// and the path still stays inside the lattice: 0 <= u <= min(d, Ub) on every diagonal
__device__ __forceinline__ void tra_backtrace(const unsigned long long *bp, int *path, int W, int D, int Ub, int lane) {
  int u = Ub, d = D - 1;
  while (d >= 0) {
    const int col = u >> 6, dj = d - lane;
    const unsigned long long wj = dj >= 1 ? bp[(size_t)dj * W + col] : 0ull;      // (diagonal 0 has no predecessor)
    const int lo = (int)(unsigned)wj, hi = (int)(unsigned)(wj >> 32);
    int mine = 0, done = 0;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      if (d - j < 0 || (u >> 6) != col) break;
      if (lane == j) mine = u;
      const unsigned long long w = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo, j) |
                                   ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, j) << 32);
      const int bit = (int)((w >> (u & 63)) & 1ull);
      u -= (u >= 1 && (bit != 0 || u == d - j)) ? 1 : 0;
      done = j + 1;
    }
    if (lane < done) path[dj] = mine;
    d -= done;
  }
}

// From the path to the outputs, all threads, behind a barrier.  Node d of the path leaves by the move its successor
// names: the label move (frame, conf) if u grows, the blank (state) otherwise; the last node leaves by the final blank.
// score: thread tid adds the terms of d = tid, tid + 256, .., then a tree over the threads
__device__ __forceinline__ void tra_finish(const TrAlignArgs &p, int b, int tid, int Tb, int Ub, const int *path) {
  __shared__ float red[TR_NT];
  const int T = p.T, U1 = p.U1, D = Tb + Ub;
  const float *lbp = p.lb + tra_slab(p, b), *lyp = p.ly + tra_slab(p, b);
  for (int t = Tb + tid; t < T; t += TR_NT) p.state[(size_t)b * T + t] = -1;
  for (int i = Ub + tid; i < U1 - 1; i += TR_NT) {
    p.frame[(size_t)b * (U1 - 1) + i] = -1;
    p.conf[(size_t)b * (U1 - 1) + i] = 0.f;
  }
  float acc = 0.f;
  for (int d = tid; d < D; d += TR_NT) {
    const int u = path[d], t = d - u;
    const bool lab = d + 1 < D && path[d + 1] != u;
    const size_t at = (size_t)d * U1 + u;
    const float x = lab ? lyp[at] : lbp[at];
    // (tra_backtrace takes existing moves only, so 0 <= u <= Ub and 0 <= t < Tb; the tests stay as a second fence)
    if (lab && u >= 0 && u < Ub) {
      p.frame[(size_t)b * (U1 - 1) + u] = t;
      p.conf[(size_t)b * (U1 - 1) + u] = x;
    } else if (!lab && t >= 0 && t < Tb) {
      p.state[(size_t)b * T + t] = u;
    }
    acc += x;
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = TR_NT / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) p.score[b] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------
// wave route: grid B, 256 threads of which wave 0 sweeps and walks back.  Dynamic LDS (IN_LDS): bp [T+U1] words of 64
// bits, path [T+U1] int
template <bool IN_LDS>
__global__ __launch_bounds__(TR_NT) void transducer_align_wave_kernel(TrAlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tra_smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = threadIdx.x & 63, U1 = p.U1;
  if (tr_lengths_labels_bad(p.T, U1, p.C, p.enc_len, p.labels, p.ldl, p.label_len, b, tid, TR_NT)) {
    tra_reject(p, b, tid);
    return;
  }
  const int Tb = p.enc_len[b], Ub = p.label_len[b], D = Tb + Ub;       // diagonals 0 .. D-1
  const int Dmax = p.T + U1;
  // (one address space per instantiation: LDS or global instructions, not flat ones)
  unsigned long long *bp = IN_LDS ? tra_smem : reinterpret_cast<unsigned long long *>(p.trace_ws + (size_t)b * p.trace_stride);
  int *path = reinterpret_cast<int *>(bp + Dmax);
  if (tid < 64) {
    const size_t slab = tra_slab(p, b);
    const int lu = lane < U1 ? lane : U1 - 1;            // (a column inside the row for the idle lanes' loads)
    const float *lbp = p.lb + slab + lu, *lyp = p.ly + slab + lu;
    const bool mine = lane <= Ub;
    // diagonal d is made from the terms of diagonal d-1: node (t-1,u) stays in its lane, node (t,u-1) hands its
    // v + ly one lane up (the alpha sweep's walk)
    float a = lane == 0 ? 0.f : TR_NEG;
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
      unsigned long long w = 0;             // lane j: the moves of diagonal d0 + j, a bit per lane
#pragma unroll
      for (int j = 0; j < TR_AHEAD; ++j) {
        const int d = d0 + j;
        if (d < D) {
          const int t = d - lane;
          const bool from = mine && t >= 1 && t <= Tb;          // node (t-1, u) exists: its terms are written
          const float emit = tr_up(a + (from ? cy[j] : TR_NEG), TR_NEG);
          bool lab;
          const float n = tra_node(a + (from ? cb[j] : TR_NEG), emit, &lab);
          const bool here = mine && t >= 0 && t < Tb;
          a = here ? n : TR_NEG;
          const unsigned long long moves = __ballot(lab && here);
          if (lane == j) w = moves;
        }
      }
      if (lane < TR_AHEAD && d0 + lane < D) bp[d0 + lane] = w;
    }
    __threadfence_block();                  // the words of the other lanes, before the backtrace reads them
    tra_backtrace(bp, path, 1, D, Ub, lane);
  }
  __threadfence_block();
  __syncthreads();
  tra_finish(p, b, tid, Tb, Ub, path);
}

// workgroup route: grid B, 256 threads.  Dynamic LDS: two rows of U1 floats (the previous diagonal and the one being
// made), then (IN_LDS) bp [(T+U1) W] words of 64 bits, path [T+U1] int
template <bool IN_LDS>
__global__ __launch_bounds__(TR_NT) void transducer_align_wg_kernel(TrAlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tra_smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = threadIdx.x & 63, U1 = p.U1, W = p.W;
  if (tr_lengths_labels_bad(p.T, U1, p.C, p.enc_len, p.labels, p.ldl, p.label_len, b, tid, TR_NT)) {
    tra_reject(p, b, tid);
    return;
  }
  const int Tb = p.enc_len[b], Ub = p.label_len[b], D = Tb + Ub;
  const int Dmax = p.T + U1;
  float *prev = reinterpret_cast<float *>(tra_smem), *cur = prev + U1;
  unsigned long long *bp = IN_LDS ? tra_smem + (U1 + 1) / 2 * 2       // (behind the rows)
                                  : reinterpret_cast<unsigned long long *>(p.trace_ws + (size_t)b * p.trace_stride);
  int *path = reinterpret_cast<int *>(bp + (size_t)Dmax * W);
  const size_t slab = tra_slab(p, b);
  const float *lbp = p.lb + slab, *lyp = p.ly + slab;
  for (int u = tid; u <= Ub; u += TR_NT) prev[u] = u == 0 ? 0.f : TR_NEG;
  __syncthreads();
  for (int d = 1; d < D; ++d) {
    for (int u0 = 0; u0 <= Ub; u0 += TR_NT) {          // (the same trips for every thread: the lane mask is whole)
      const int u = u0 + tid;
      bool lab = false, here = false;
      if (u <= Ub) {
        const int t = d - u;
        const bool from = t >= 1 && t <= Tb;
        float emit = TR_NEG;                                     // (the fill of the wave route's shift)
        if (u >= 1) {
          const bool lfrom = t >= 0 && t < Tb;                   // node (t, u-1) exists
          emit = prev[u - 1] + (lfrom ? lyp[(size_t)(d - 1) * U1 + u - 1] : TR_NEG);
        }
        const float n = tra_node(prev[u] + (from ? lbp[(size_t)(d - 1) * U1 + u] : TR_NEG), emit, &lab);
        here = t >= 0 && t < Tb;
        cur[u] = here ? n : TR_NEG;
      }
      const unsigned long long moves = __ballot(lab && here);
      if (lane == 0 && u <= Ub) bp[(size_t)d * W + (u >> 6)] = moves;
    }
    __syncthreads();
    float *tmp = prev; prev = cur; cur = tmp;
  }
  __threadfence_block();
  __syncthreads();
  if (tid < 64) tra_backtrace(bp, path, W, D, Ub, lane);
  __threadfence_block();
  __syncthreads();
  tra_finish(p, b, tid, Tb, Ub, path);
}

static size_t tra_nodes(int B, int T, int U1) { return (size_t)B * ((size_t)T + U1) * U1; }
static int tra_words(int U1) { return (U1 + 63) / 64; }
// back-pointers and path of one utterance (the workgroup route's W: the wave route's is 1, which is no more)
static size_t tra_trace_bytes(int T, int U1) { return ((size_t)T + U1) * ((size_t)tra_words(U1) * 8 + 4); }
static size_t tra_trace_stride(int T, int U1) { return align_up(tra_trace_bytes(T, U1), 16); }
static size_t tra_wg_rows(int U1) { return (size_t)((U1 + 1) / 2 * 2) * 2 * sizeof(float); }     // (keeps bp 8-byte aligned)

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_transducer_align_ws_bytes(int B, int T, int U1) {
  if (B <= 0 || T <= 0 || U1 <= 0) return 0;
  return 2 * align_up(tra_nodes(B, T, U1) * sizeof(float), 16) + (size_t)B * tra_trace_stride(T, U1);
}

extern "C" size_t nabu_transducer_align_lds_bytes(int T, int U1, int workgroup_route) {
  if (T <= 0 || U1 <= 0) return 0;
  return workgroup_route ? tra_wg_rows(U1) + tra_trace_bytes(T, U1) : ((size_t)T + U1) * (8 + 4);
}

extern "C" int nabu_transducer_align(int B, int T, int U1, int C, const float *f, const float *g,
                                     const int32_t *enc_len, const int32_t *labels, int ldl,
                                     const int32_t *label_len, int32_t *state, int32_t *frame, float *conf,
                                     float *score, int32_t *status, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && U1 > 0 && C > 1, "transducer_align: bad dimensions");
  NABU_CHECK_ARG(f && g && enc_len && label_len && state && score && status && ws, "transducer_align: null pointer");
  NABU_CHECK_ARG(U1 == 1 || (frame && conf), "transducer_align: null frame or conf");
  NABU_CHECK_ARG(U1 == 1 || (labels && ldl >= U1 - 1), "transducer_align: null labels or ldl < U1 - 1");
  NABU_CHECK_ARG((size_t)T * U1 < ((size_t)1 << 31) && (size_t)B * ((size_t)T + U1) < ((size_t)1 << 31),
                 "transducer_align: T * U1 or B * (T + U1) does not fit an int");
  const size_t need = nabu_transducer_align_ws_bytes(B, T, U1);
  if (ws_bytes < need) return fail(NABU_EWS, "transducer_align: workspace %zu < %zu", ws_bytes, need);
  static const int force_wg = env_int("NABU_TRANSDUCER_ALIGN_WORKGROUP", 0);   // 1: the workgroup route for every shape (A/B tests)
  const bool wave = !force_wg && U1 <= 64;
  constexpr size_t LDS_MAX = 150 * 1024;
  const size_t rows = wave ? 0 : tra_wg_rows(U1);
  if (rows > LDS_MAX) return fail(NABU_EUNSUP, "transducer_align: U1=%d needs %zu B of LDS", U1, rows);
  const size_t all = nabu_transducer_align_lds_bytes(T, U1, wave ? 0 : 1);
  const bool in_lds = all <= LDS_MAX;            // back-pointers and path in LDS while they fit
  const size_t shm = in_lds ? all : rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  TrAlignArgs p;
  p.B = B; p.T = T; p.U1 = U1; p.C = C; p.ldl = ldl; p.W = wave ? 1 : tra_words(U1);
  p.f = f; p.g = g; p.enc_len = enc_len; p.labels = labels; p.label_len = label_len;
  p.state = state; p.frame = frame; p.conf = conf; p.score = score; p.status = status;
  const size_t arr = align_up(tra_nodes(B, T, U1) * sizeof(float), 16) / sizeof(float);
  float *w = static_cast<float *>(ws);
  p.lb = w; p.ly = w + arr;
  p.trace_ws = reinterpret_cast<unsigned char *>(w + 2 * arr);
  p.trace_stride = tra_trace_stride(T, U1);
  // measurement only (tools/transducer_align_bench.py): a mask of the launches to make — 1 emission terms, 2 sweep and
  // backtrace — on a workspace that a complete call with the same operands has filled.  Read on every call
  const int todo = env_int("NABU_TRANSDUCER_ALIGN_LAUNCHES", 3);
  NABU_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (todo & 1) {
    hipLaunchKernelGGL(transducer_align_emit_kernel, dim3((T * U1 + TR_NT - 1) / TR_NT, B), dim3(TR_NT), 0, s, p);
    NABU_LAUNCH_CHECK();
  }
  if (!(todo & 2)) return 0;
  if (wave)
    return in_lds ? launch_lds(transducer_align_wave_kernel<true>, dim3(B), dim3(TR_NT), shm, s, p)
                  : launch_lds(transducer_align_wave_kernel<false>, dim3(B), dim3(TR_NT), shm, s, p);
  return in_lds ? launch_lds(transducer_align_wg_kernel<true>, dim3(B), dim3(TR_NT), shm, s, p)
                : launch_lds(transducer_align_wg_kernel<false>, dim3(B), dim3(TR_NT), shm, s, p);
}
