// ctc_align.hip — forced alignment with a CTC model: the best path through the label lattice the loss sums over
// (ctc.hip), its per-label segments, confidences and score.  Contract: include/nabu_hip.h, nabu_ctc_align.
//
// A max-plus sweep on the RAW logits (every path visits every frame once, so the frame normalisers cannot change the
// arg-max: no exp or log in the frame loop, and ties are exact), a back-pointer of 2 bits (wave route) or a byte
// (workgroup route) per (frame, state), a backtrace by one lane, and an epilogue over all threads that turns the path
// into state / seg / conf / score.  The log-softmax is evaluated only along the path; its frame normalisers do not
// depend on the path, and the wave route's idle waves work them out beside the sweep.
//
// Two routes, as in ctc.hip:
//   wave       Lmax <= 63 (S <= 127): ONE wave64 runs the sweep, lane i owns the state pair (blank 2i, label 2i+1);
//              the one neighbour value a frame needs comes through a DPP wave shift, so the frame loop has no barrier
//              and no LDS traffic.  The two emissions a lane needs per frame are gathered 16 .. 32 frames ahead into
//              registers; the 16 frames' back-pointers (4 bits each) leave as one 64-bit word per lane.
//   workgroup  everything else: 256 threads, states strided over the threads (S may exceed 256), ping-pong rows in
//              LDS, one barrier per frame; the emissions of a thread's first two states are gathered 4 .. 8 frames
//              ahead.
// Back-pointers live in LDS while they fit beside the path and the frame terms, in the caller's workspace otherwise.
#include <stdlib.h>

#include "common.h"

namespace nabu {

constexpr float ALN_NEG = -1e30f;   // unreachable (CTC_NEG of ctc.hip): -1e30 + x is -1e30 again, never inf - inf
constexpr int ALN_NT = 256;
constexpr int ALN_CHUNK = 16;       // frames per back-pointer word of the wave route

struct AlignArgs {
  int B, T, C, Lmax, Smax;
  const float *logits;
  const int32_t *logit_len, *labels, *label_len;
  int32_t *state, *seg;
  float *conf, *score;
  int32_t *status;
  unsigned char *bp_ws;      // workspace back-pointers, bp_stride bytes per utterance
  size_t bp_stride;
};

__device__ __forceinline__ float aln_up(float v, float fill) {     // lane i <- lane i-1 (lane 0 <- fill)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// a frame's maximum and log sum exp(x - maximum)
__device__ __forceinline__ void frame_lse(const float *x, int C, float *mx, float *lz) {
  float m = x[0];
  for (int k = 1; k < C; ++k) m = fmaxf(m, x[k]);
  float z = 0.f;
  for (int k = 0; k < C; ++k) z += expf(x[k] - m);
  *mx = m;
  *lz = logf(z);
}

// an utterance without a valid alignment: score -inf, state / seg -1, conf 0, and its number in the status word
__device__ void align_reject(const AlignArgs &p, int b, int tid) {
  for (int t = tid; t < p.T; t += ALN_NT) p.state[(size_t)b * p.T + t] = -1;
  for (int i = tid; i < p.Lmax; i += ALN_NT) {
    p.seg[((size_t)b * p.Lmax + i) * 2] = -1;
    p.seg[((size_t)b * p.Lmax + i) * 2 + 1] = -1;
    p.conf[(size_t)b * p.Lmax + i] = 0.f;
  }
  if (tid == 0) {
    p.score[b] = -__builtin_inff();
    // the loss's atomicCAS(status, 0, b + 1), repeated while a LATER utterance holds the word: the status names the
    // first bad utterance of the batch whichever workgroup comes first, so it is as reproducible as the other outputs
    const int want = b + 1;
    int old = atomicCAS(p.status, 0, want);
    while (old != 0 && old > want) {
      const int seen = atomicCAS(p.status, old, want);
      if (seen == old) break;
      old = seen;
    }
  }
}

// From the path st[0 .. Tb) (LDS) to the outputs, all threads, behind a barrier:
//   frame per thread   term[t] = (x[c_t] - mx) - lz, state, and the segment ends a frame sees
//   score              term summed in a fixed order: thread tid adds t = tid, tid + 256, .., then a tree over the threads
//   label per thread   seg and conf (the mean of term over the segment, added in frame order)
// PRE: the frames' maxima (fmx) and log-sums (in term) are there already (the wave route's idle waves compute them
// beside the sweep); the expressions are the same either way, so both routes give the same bits
template <bool PRE>
__device__ void align_finish(const AlignArgs &p, int b, int tid, int Tb, int L, const int *st, float *term, int *segl,
                             const float *fmx) {
  __shared__ float red[ALN_NT];
  const int T = p.T, C = p.C, blank = p.C - 1;
  const float *lg = p.logits + (size_t)b * T * C;
  for (int t = tid; t < T; t += ALN_NT) {
    int s = -1;
    if (t < Tb) {
      s = st[t];
      const int c = (s & 1) ? p.labels[(size_t)b * p.Lmax + (s >> 1)] : blank;
      const float *x = lg + (size_t)t * C;
      float m, lz;
      if (PRE) {
        m = fmx[t];
        lz = term[t];
      } else {
        frame_lse(x, C, &m, &lz);
      }
      term[t] = (x[c] - m) - lz;               // kept apart as in ctc_kernel
      if (s & 1) {
        if (t == 0 || st[t - 1] != s) segl[s - 1] = t;            // segl[2i], i = s >> 1
        if (t == Tb - 1 || st[t + 1] != s) segl[s] = t + 1;       // segl[2i + 1]
      }
    }
    p.state[(size_t)b * T + t] = s;
  }
  __syncthreads();
  float acc = 0.f;
  for (int t = tid; t < Tb; t += ALN_NT) acc += term[t];
  red[tid] = acc;
  __syncthreads();
  for (int o = ALN_NT / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) p.score[b] = red[0];
  for (int i = tid; i < p.Lmax; i += ALN_NT) {
    int a = -1, e = -1;
    float cf = 0.f;
    if (i < L) {
      a = segl[2 * i];
      e = segl[2 * i + 1];
      for (int t = a; t < e; ++t) cf += term[t];
      cf /= (float)(e - a);
    }
    p.seg[((size_t)b * p.Lmax + i) * 2] = a;
    p.seg[((size_t)b * p.Lmax + i) * 2 + 1] = e;
    p.conf[(size_t)b * p.Lmax + i] = cf;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// wave route.  LDS: st [T] int, term [T] float, fmx [T (+1)] float, segl [128] int, then (BP_LDS) ceil(T/16) * 64 words
// of 64 bits.  While wave 0 sweeps and walks back, the other three waves work out every frame's maximum and log-sum —
// they do not depend on the path — so the epilogue is left with one subtraction per frame.
template <bool BP_LDS>
__global__ __launch_bounds__(ALN_NT) void ctc_align_wave_kernel(AlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int T = p.T, C = p.C, blank = p.C - 1;
  int *st = reinterpret_cast<int *>(smem);
  float *term = smem + T;
  float *fmx = term + T;
  int *segl = reinterpret_cast<int *>(fmx + T + (T & 1));      // (keeps the 64-bit words behind it aligned)
  // (one address space per instantiation: LDS or global instructions, not flat ones)
  unsigned long long *bp = BP_LDS ? reinterpret_cast<unsigned long long *>(segl + 128)
                                  : reinterpret_cast<unsigned long long *>(p.bp_ws + (size_t)b * p.bp_stride);
  int Tb = p.logit_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int L = p.label_len[b];
  L = L < 0 ? 0 : (L > p.Lmax ? p.Lmax : L);
  const float *lg = p.logits + (size_t)b * T * C;

  // every wave reaches the same verdict from the same labels
  const int lab = lane < L ? p.labels[(size_t)b * p.Lmax + lane] : -1;
  const int lab_prev = __shfl_up(lab, 1, 64);
  const int lab_up = lane >= 1 ? lab_prev : -1;
  const bool badl = lane < L && (lab < 0 || lab >= blank);
  const int rep = (int)wave_sum((lane >= 1 && lane < L && lab == lab_up) ? 1.f : 0.f);
  if (__any(badl) || Tb <= 0 || L + rep > Tb) {     // ctc_kernel's test
    align_reject(p, b, tid);
    return;
  }
  if (wv == 0) {
    const bool hasB = lane <= L, hasL = lane < L;
    const bool skipA = lane >= 1 && hasL && lab != lab_up;    // 2i-1 -> 2i+1
    const float *colB = lg + blank, *colL = lg + (hasL ? lab : blank);   // (a valid column for idle lanes)
    // the emissions of a chunk are loaded one chunk ahead: independent of the recursion, in flight while it runs.
    // The blank's, the same for every lane, come as ONE load per chunk — lane j holds frame j's — and are read with
    // v_readlane (left as 16 uniform loads the compiler makes them scalar loads and sinks each to its use: a scalar
    // cache round trip on every frame of the chain)
    const int jl = lane & (ALN_CHUNK - 1);
    float nbv, nl[ALN_CHUNK];
    nbv = colB[(size_t)(jl < Tb ? jl : Tb - 1) * C];
#pragma unroll
    for (int j = 0; j < ALN_CHUNK; ++j) {
      const int tt = j < Tb ? j : Tb - 1;
      nl[j] = colL[(size_t)tt * C];
    }
    float vB = ALN_NEG, vL = ALN_NEG;
    for (int t0 = 0; t0 < Tb; t0 += ALN_CHUNK) {
      float cl[ALN_CHUNK];
      const float cbv = nbv;
#pragma unroll
      for (int j = 0; j < ALN_CHUNK; ++j) cl[j] = nl[j];
      {
        const int tt = t0 + ALN_CHUNK + jl;
        nbv = colB[(size_t)(tt < Tb ? tt : Tb - 1) * C];
      }
#pragma unroll
      for (int j = 0; j < ALN_CHUNK; ++j) {
        int tt = t0 + ALN_CHUNK + j;
        tt = tt < Tb ? tt : Tb - 1;
        nl[j] = colL[(size_t)tt * C];
      }
      unsigned long long w = 0;
#pragma unroll
      for (int j = 0; j < ALN_CHUNK; ++j) {
        const int t = t0 + j;
        if (t < Tb) {
          const float yB = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cbv), j));
          if (t == 0) {
            vB = lane == 0 ? yB : ALN_NEG;
            vL = (lane == 0 && hasL) ? cl[j] : ALN_NEG;
          } else {
            const float up = aln_up(vL, ALN_NEG);            // v[2i-1]
            // a tie keeps the smaller move: step only if strictly greater than stay, skip only if greater than both
            const bool stepB = up > vB;
            const float mB = stepB ? up : vB;
            float mL = vL;
            unsigned kL = 0;
            if (vB > mL) { mL = vB; kL = 1; }
            if (skipA && up > mL) { mL = up; kL = 2; }
            vB = hasB ? mB + yB : ALN_NEG;
            vL = hasL ? mL + cl[j] : ALN_NEG;
            w |= (unsigned long long)((stepB ? 1u : 0u) | (kL << 2)) << (4 * j);
          }
        }
      }
      bp[(size_t)(t0 / ALN_CHUNK) * 64 + lane] = w;
    }
    // the end rule: state S-1 unless S-2 is strictly better
    const float endB = __shfl(vB, L, 64);
    const float endL = __shfl(vL, L >= 1 ? L - 1 : 0, 64);
    __threadfence_block();                    // the back-pointers of the other lanes, before lane 0 reads them
    if (lane == 0) {
      int s = (L >= 1 && endL > endB) ? 2 * L - 1 : 2 * L;
      size_t have = ~(size_t)0;
      unsigned long long w = 0;
      for (int t = Tb - 1; t >= 0; --t) {
        st[t] = s;
        const size_t at = (size_t)(t / ALN_CHUNK) * 64 + (s >> 1);
        if (at != have) {                     // (a path that stays with a lane re-uses the word it has)
          w = bp[at];
          have = at;
          // the wait for the word belongs in here: at the join it would also wait for the store of st[t], every frame
          asm volatile("" : "+v"(w));
        }
        s -= (int)((w >> (4 * (t % ALN_CHUNK) + 2 * (s & 1))) & 3u);
      }
    }
  } else {
    for (int t = tid - 64; t < Tb; t += ALN_NT - 64) frame_lse(lg + (size_t)t * C, C, fmx + t, term + t);
  }
  __syncthreads();
  align_finish<true>(p, b, tid, Tb, L, st, term, segl, fmx);
}

// ---------------------------------------------------------------------------------------------------------------
// workgroup route.  LDS: st [T] int, term [T] float, segl [2 max(Lmax, 1)] int, row0, row1 [Smax] float, ext [Smax] int,
// then (bp_lds) T * Smax bytes
template <bool BP_LDS>
__global__ __launch_bounds__(ALN_NT) void ctc_align_wg_kernel(AlignArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int s_bad;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = p.T, C = p.C, Smax = p.Smax, blank = p.C - 1;
  int *st = reinterpret_cast<int *>(smem);
  float *term = smem + T;
  int *segl = reinterpret_cast<int *>(term + T);
  float *row0 = reinterpret_cast<float *>(segl + 2 * (p.Lmax > 0 ? p.Lmax : 1));
  float *row1 = row0 + Smax;
  int *ext = reinterpret_cast<int *>(row1 + Smax);
  unsigned char *bp = BP_LDS ? reinterpret_cast<unsigned char *>(ext + Smax) : p.bp_ws + (size_t)b * p.bp_stride;
  int Tb = p.logit_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int L = p.label_len[b];
  L = L < 0 ? 0 : (L > p.Lmax ? p.Lmax : L);
  const int S = 2 * L + 1;
  const float *lg = p.logits + (size_t)b * T * C;

  for (int s = tid; s < S; s += ALN_NT) ext[s] = (s & 1) ? p.labels[(size_t)b * p.Lmax + (s >> 1)] : blank;
  __syncthreads();
  if (tid == 0) {
    int rep = 0, bad = 0;
    for (int i = 0; i < L; ++i) {
      const int l = ext[2 * i + 1];
      if (l < 0 || l >= blank) bad = 1;
      if (i > 0 && l == ext[2 * i - 1]) ++rep;
    }
    if (Tb <= 0 || L + rep > Tb) bad = 1;       // ctc_kernel's test
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad) {
    align_reject(p, b, tid);
    return;
  }
  float *prev = row0, *cur = row1;
  for (int s = tid; s < S; s += ALN_NT) prev[s] = s < 2 ? lg[ext[s]] : ALN_NEG;
  // the emissions of a thread's first two states, four frames per group, loaded one group ahead
  const float *col0 = lg + (tid < S ? ext[tid] : blank), *col1 = lg + (tid + ALN_NT < S ? ext[tid + ALN_NT] : blank);
  float n0[4], n1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int tt = 1 + j < Tb ? 1 + j : Tb - 1;
    n0[j] = col0[(size_t)tt * C];
    n1[j] = col1[(size_t)tt * C];
  }
  __syncthreads();
  for (int t0 = 1; t0 < Tb; t0 += 4) {
    float c0[4], c1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c0[j] = n0[j];
      c1[j] = n1[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int tt = t0 + 4 + j;
      tt = tt < Tb ? tt : Tb - 1;
      n0[j] = col0[(size_t)tt * C];
      n1[j] = col1[(size_t)tt * C];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j;
      if (t < Tb) {                            // (the same for every thread: the barrier is reached by all or none)
        for (int s = tid, k = 0; s < S; s += ALN_NT, ++k) {
          const int e = ext[s];
          const float x = k == 0 ? c0[j] : (k == 1 ? c1[j] : lg[(size_t)t * C + e]);
          float m = prev[s];
          unsigned char kk = 0;
          if (s >= 1) {
            const float a1 = prev[s - 1];
            if (a1 > m) { m = a1; kk = 1; }
          }
          if ((s & 1) && s >= 3 && e != ext[s - 2]) {
            const float a2 = prev[s - 2];
            if (a2 > m) { m = a2; kk = 2; }
          }
          cur[s] = m + x;
          bp[(size_t)t * Smax + s] = kk;
        }
        __syncthreads();
        float *tmp = prev; prev = cur; cur = tmp;
      }
    }
  }
  if (tid == 0) {
    int s = (S >= 2 && prev[S - 2] > prev[S - 1]) ? S - 2 : S - 1;
    for (int t = Tb - 1; t >= 0; --t) {
      st[t] = s;
      if (t > 0) s -= bp[(size_t)t * Smax + s];
    }
  }
  __syncthreads();
  align_finish<false>(p, b, tid, Tb, L, st, term, segl, nullptr);
}

// LDS beside the back-pointers, and the back-pointers of one utterance, per route
static size_t align_wave_base(int T) { return ((size_t)3 * T + (T & 1) + 128) * 4; }
static size_t align_wave_bp(int T) { return (size_t)((T + ALN_CHUNK - 1) / ALN_CHUNK) * 64 * 8; }
static size_t align_wg_base(int T, int Lmax) {
  return ((size_t)2 * T + 2 * (size_t)(Lmax > 0 ? Lmax : 1) + 3 * (2 * (size_t)Lmax + 1)) * 4;
}
static size_t align_wg_bp(int T, int Lmax) { return (size_t)T * (2 * (size_t)Lmax + 1); }
static size_t align_bp_stride(int T, int Lmax) {
  const size_t a = align_wave_bp(T), c = align_wg_bp(T, Lmax);
  return align_up(a > c ? a : c, 16);
}

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_ctc_align_ws_bytes(int B, int T, int Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0) return 0;
  return (size_t)B * align_bp_stride(T, Lmax);
}

extern "C" int nabu_ctc_align(int B, int T, int C, int Lmax, const float *logits, const int32_t *logit_len,
                              const int32_t *labels, const int32_t *label_len, int32_t *state, int32_t *seg,
                              float *conf, float *score, int32_t *status, void *ws, size_t ws_bytes,
                              nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && C > 1 && Lmax >= 0, "ctc_align: bad dimensions");
  NABU_CHECK_ARG(logits && logit_len && label_len && state && seg && conf && score && status && ws,
                 "ctc_align: null pointer");
  NABU_CHECK_ARG(Lmax == 0 || labels, "ctc_align: null labels");
  const size_t need = nabu_ctc_align_ws_bytes(B, T, Lmax);
  if (ws_bytes < need) return fail(NABU_EWS, "ctc_align: workspace %zu < %zu", ws_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  AlignArgs p;
  p.B = B; p.T = T; p.C = C; p.Lmax = Lmax; p.Smax = 2 * Lmax + 1;
  p.logits = logits; p.logit_len = logit_len; p.labels = labels; p.label_len = label_len;
  p.state = state; p.seg = seg; p.conf = conf; p.score = score; p.status = status;
  p.bp_ws = static_cast<unsigned char *>(ws);
  p.bp_stride = align_bp_stride(T, Lmax);
  static const int force_wg = env_int("NABU_CTC_ALIGN_WORKGROUP", 0);   // 1: the workgroup route for every shape (A/B tests)
  constexpr size_t LDS_MAX = 150 * 1024;
  const bool wave = !force_wg && Lmax <= 63 && align_wave_base(T) <= LDS_MAX;
  const size_t base = wave ? align_wave_base(T) : align_wg_base(T, Lmax);
  const size_t bpb = wave ? align_wave_bp(T) : align_wg_bp(T, Lmax);
  if (base > LDS_MAX)
    return fail(NABU_EUNSUP, "ctc_align: T=%d, Lmax=%d need %zu B of LDS", T, Lmax, base);
  const bool bp_lds = base + bpb <= LDS_MAX;       // back-pointers in LDS while they fit
  const size_t shm = bp_lds ? base + bpb : base;
  NABU_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  if (wave)
    return bp_lds ? launch_lds(ctc_align_wave_kernel<true>, dim3(B), dim3(ALN_NT), shm, s, p)
                  : launch_lds(ctc_align_wave_kernel<false>, dim3(B), dim3(ALN_NT), shm, s, p);
  return bp_lds ? launch_lds(ctc_align_wg_kernel<true>, dim3(B), dim3(ALN_NT), shm, s, p)
                : launch_lds(ctc_align_wg_kernel<false>, dim3(B), dim3(ALN_NT), shm, s, p);
}
