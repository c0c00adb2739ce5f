// ctc_prefix.hip — CTC prefix scores for the joint CTC/attention beam search (Watanabe et al. 2017, "Hybrid
// CTC/attention architecture for end-to-end speech recognition", Algorithm 2 in the log domain).
//
// For a hypothesis g (labels without the start symbol) of utterance b with T = enc_len[b] frames, the state is two
// log-space vectors over the frames,
//   r_n(t, g): all paths of frames 0..t that collapse to g and end in a label,
//   r_b(t, g): ... and end in the blank,
// kept as (r_n, r_b) pairs in state[B, W, T, 2], with psi[B, W] = log P_ctc(g . anything) and last[B, W] = g's final
// label (-1: g is empty).  y_t(k) = (x[t,k] - mx[t]) - lz[t] is the log-softmax of the head's logits, from the frame
// maximum and the log of the sum that prepare leaves in norm[B, T, 2] (kept apart as in ctc.hip: a frame whose
// winner has probability ~1 keeps its small -log p).  The blank is C-1, which is also the Speller's end label.
//
//   prepare  once per search: norm, and the state of the empty hypothesis in all W slots (one workgroup per utterance)
//   score    per step: delta[b,w,c] = psi(g.c) - psi(g) for all C classes (one workgroup per (b, w), a thread per
//            class).  psi(g.c) needs only phi_t — r_b(t-1,g), or r_n (+) r_b when c differs from g's last label — and
//            y_t(c): the workgroup builds both phi vectors once in LDS and every thread sums its class over the
//            frames (running maximum + sum of exponentials), its logits fetched eight frames ahead.
//   advance  per step, after pruning: the W survivors' states.  RECOMPUTED, one hypothesis per wave, where keeping
//            the states of all W*C candidates would cost [B,W,C,T,2] floats per step (20 MB at B 32, W 16, C 40,
//            T 125): the wave stages phi, y(pred) and y(blank) of all frames in LDS in parallel and runs the two
//            recurrences as scans over the frames (wave_recurrence), r_b after r_n, which it reads.
// log 0 is CTC_NEG, the finite stand-in of ctc.hip, so no inf - inf arises; a hypothesis that does not fit into its
// utterance has psi = CTC_NEG, and so has every extension of it (delta 0 from there on).
#include "common.h"

namespace nabu {

namespace {
constexpr float CTC_NEG = -1e30f;   // ctc.hip's log 0
constexpr int AHEAD = 8;            // frames of logits a class thread of the score kernel holds in registers

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  return m + log1pf(expf(n - m));
}
__device__ __forceinline__ float floor_neg(float v) { return fmaxf(v, CTC_NEG); }
__device__ __forceinline__ int clamp_len(int t, int T) { return t < 0 ? 0 : (t > T ? T : t); }

// x -> lse(x + a, b): one frame of a prefix recurrence.  Such maps compose — first f, then g, is
// (f.a + g.a, lse(f.b + g.a, g.b)) — so a wave runs a T-frame recurrence as a scan instead of a chain of T dependent
// log-sum-exps: every lane composes the maps of its own run of ceil((T-1)/64) consecutive frames, six exchange steps
// turn them into prefixes over the lanes, and every lane walks its run from the value the prefix before it gives.
struct Aff { float a, b; };
__device__ __forceinline__ Aff aff_then(Aff f, Aff g) { return Aff{f.a + g.a, lse2(f.b + g.a, g.b)}; }
// rec(t) = floor(lse(rec(t-1) + a(t), b(t))) for 1 <= t < Tb from rec(0) = r0, handed to out(t, rec(t)); Tb >= 1, one wave
template <typename FA, typename FB, typename Out>
__device__ __forceinline__ void wave_recurrence(int Tb, float r0, FA a, FB b, Out out) {
  const int lane = threadIdx.x & 63, n = (Tb - 1 + 63) / 64;
  const int t0 = 1 + lane * n, t1 = t0 + n < Tb ? t0 + n : Tb;
  Aff f = {0.f, CTC_NEG};                        // the identity
  for (int t = t0; t < t1; ++t) f = aff_then(f, Aff{a(t), b(t)});
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Aff prev = {__shfl_up(f.a, o, 64), __shfl_up(f.b, o, 64)};
    if (lane >= o) f = aff_then(prev, f);
  }
  const Aff before = {__shfl_up(f.a, 1, 64), __shfl_up(f.b, 1, 64)};
  float v = lane == 0 ? r0 : floor_neg(lse2(r0 + before.a, before.b));
  for (int t = t0; t < t1; ++t) {
    v = floor_neg(lse2(v + a(t), b(t)));
    out(t, v);
  }
}

struct PrefixArgs {
  int B, W, T, C;
  const float *logits;          // [B,T,C]
  const int32_t *enc_len;       // [B]
  float *norm;                  // [B,T,2]  (mx, lz)
  const float *state_in;        // [B,W,T,2]
  const float *psi_in;          // [B,W]
  const int32_t *last_in;       // [B,W]
  const int32_t *finished, *parent, *stay, *pred;
  float *state_out, *psi_out, *delta;
  int32_t *last_out;
};

// one workgroup of 256 threads per utterance; LDS: T floats
__global__ __launch_bounds__(256) void ctc_prefix_prepare_kernel(PrefixArgs p) {
  extern __shared__ __attribute__((aligned(16))) float cum[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, T = p.T, C = p.C, W = p.W;
  const int Tb = clamp_len(p.enc_len[b], T);
  const float *x0 = p.logits + (size_t)b * T * C;
  float2 *norm = reinterpret_cast<float2 *>(p.norm) + (size_t)b * T;
  for (int t = tid >> 6; t < T; t += 4) {
    if (t >= Tb) {
      if (lane == 0) norm[t] = make_float2(0.f, 0.f);
      continue;
    }
    const float *x = x0 + (size_t)t * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
    const float lz = logf(wave_sum(s));
    if (lane == 0) {
      norm[t] = make_float2(m, lz);
      cum[t] = (x[C - 1] - m) - lz;
    }
  }
  __syncthreads();
  if (tid == 0) {      // r_b(t, empty) = sum of y(blank) up to t: one fixed order
    float a = 0.f;
    for (int t = 0; t < Tb; ++t) { a += cum[t]; cum[t] = floor_neg(a); }
  }
  __syncthreads();
  float2 *st = reinterpret_cast<float2 *>(p.state_out) + (size_t)b * W * T;
  for (int i = tid; i < W * T; i += 256) {
    const int t = i % T;
    st[i] = make_float2(CTC_NEG, t < Tb ? cum[t] : CTC_NEG);
  }
  for (int w = tid; w < W; w += 256) {
    p.psi_out[(size_t)b * W + w] = 0.f;
    p.last_out[(size_t)b * W + w] = -1;
  }
}

// one workgroup per hypothesis (b, w), a thread per class (a loop when C exceeds the block); LDS: 4 T floats
__global__ __launch_bounds__(256) void ctc_prefix_score_kernel(PrefixArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  __shared__ float s_end;
  const int bw = blockIdx.x, b = bw / p.W, tid = threadIdx.x, nt = blockDim.x, T = p.T, C = p.C;
  float *d = p.delta + (size_t)bw * C;
  if (p.finished[bw]) {                       // its state is not read; the joint prune does not read its row either
    for (int c = tid; c < C; c += nt) d[c] = 0.f;
    return;
  }
  const int Tb = clamp_len(p.enc_len[b], T);
  float *phi_d = sm, *phi_s = sm + T, *mx = sm + 2 * T, *lz = sm + 3 * T;
  const float2 *st = reinterpret_cast<const float2 *>(p.state_in) + (size_t)bw * T;
  const float2 *norm = reinterpret_cast<const float2 *>(p.norm) + (size_t)b * T;
  for (int t = tid; t < Tb; t += nt) {
    const float2 r = st[t], n = norm[t];
    const float both = lse2(r.x, r.y);
    if (t + 1 < Tb) { phi_d[t + 1] = both; phi_s[t + 1] = r.y; }
    else s_end = both;
    mx[t] = n.x; lz[t] = n.y;
  }
  __syncthreads();
  const int last = p.last_in[bw];
  const float psi_g = p.psi_in[bw];
  for (int c = tid; c < C; c += nt) {
    float v;
    if (Tb == 0) {
      v = (c == C - 1 && last < 0) ? 0.f : CTC_NEG;
    } else if (c == C - 1) {
      v = s_end;                                // psi(g . eos) = r_n(T-1, g) (+) r_b(T-1, g)
    } else {
      const float *x = p.logits + (size_t)b * T * C + c;
      const float *phi = c == last ? phi_s : phi_d;
      // psi = r_n(0,h) (+) sum_t (phi_t + y_t(c)): a log-sum-exp over the frames, taken as a running maximum M and a
      // sum S of exp(. - M) eight frames at a time — eight independent exponentials per step of the dependent chain
      // where a chain of two-term log-sum-exps has two dependent library calls per frame
      float M = last < 0 ? (x[0] - mx[0]) - lz[0] : CTC_NEG, S = 1.f;
      float nxt[AHEAD];
#pragma unroll
      for (int j = 0; j < AHEAD; ++j) nxt[j] = 1 + j < Tb ? x[(size_t)(1 + j) * C] : 0.f;
      for (int t0 = 1; t0 < Tb; t0 += AHEAD) {
        float cur[AHEAD], u[AHEAD];
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) {
          cur[j] = nxt[j];
          const int t = t0 + AHEAD + j;
          nxt[j] = t < Tb ? x[(size_t)t * C] : 0.f;
        }
        float m8 = -INFINITY;
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) {
          const int t = t0 + j;
          u[j] = t < Tb ? phi[t] + ((cur[j] - mx[t]) - lz[t]) : -INFINITY;     // (past the end: exp(-inf - M) = 0)
          m8 = fmaxf(m8, u[j]);
        }
        if (m8 > M) { S *= expf(M - m8); M = m8; }
        float s8 = 0.f;
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) s8 += expf(u[j] - M);
        S += s8;
      }
      v = M + logf(S);
    }
    d[c] = floor_neg(v) - psi_g;
  }
}

// one wave per survivor (b, k); LDS: 4 T floats
__global__ __launch_bounds__(64) void ctc_prefix_advance_kernel(PrefixArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int bk = blockIdx.x, b = bk / p.W, lane = threadIdx.x, T = p.T, C = p.C;
  const int par = p.parent[bk], c = p.pred[bk];
  const bool stay = p.stay[bk] != 0;
  if (par < 0 || par >= p.W || c < 0 || c >= C) return;      // (never from nabu_beam_prune_joint)
  const int src = b * p.W + par;
  const int Tb = clamp_len(p.enc_len[b], T);
  const float2 *si = reinterpret_cast<const float2 *>(p.state_in) + (size_t)src * T;
  float2 *so = reinterpret_cast<float2 *>(p.state_out) + (size_t)bk * T;
  const int last = p.last_in[src];
  if (stay || c == C - 1) {
    for (int t = lane; t < T; t += 64) so[t] = si[t];
    if (lane == 0) {
      float psi = p.psi_in[src];
      if (!stay) {
        if (Tb > 0) { const float2 r = si[Tb - 1]; psi = floor_neg(lse2(r.x, r.y)); }
        else psi = last < 0 ? 0.f : CTC_NEG;
      }
      p.psi_out[bk] = psi;
      p.last_out[bk] = last;
    }
    return;
  }
  float *phi = sm, *yc = sm + T, *yb = sm + 2 * T, *rn = sm + 3 * T;
  const float *x = p.logits + (size_t)b * T * C;
  const float2 *norm = reinterpret_cast<const float2 *>(p.norm) + (size_t)b * T;
  for (int t = lane; t < T; t += 64) {
    if (t >= Tb) { so[t] = make_float2(CTC_NEG, CTC_NEG); continue; }
    const float2 r = si[t], n = norm[t];
    if (t + 1 < Tb) phi[t + 1] = c == last ? r.y : lse2(r.x, r.y);
    yc[t] = (x[(size_t)t * C + c] - n.x) - n.y;
    yb[t] = (x[(size_t)t * C + C - 1] - n.x) - n.y;
  }
  __syncthreads();
  if (Tb == 0) {
    if (lane == 0) { p.psi_out[bk] = CTC_NEG; p.last_out[bk] = c; }
    return;
  }
  // r_n(t,h) = lse(r_n(t-1,h) + y_t(c), phi_t + y_t(c)) from r_n(0,h); psi = r_n(0,h) (+) sum_t (phi_t + y_t(c))
  const float r0 = last < 0 ? yc[0] : CTC_NEG;
  if (lane == 0) rn[0] = r0;
  wave_recurrence(Tb, r0, [&](int t) { return yc[t]; }, [&](int t) { return phi[t] + yc[t]; },
                  [&](int t, float v) { rn[t] = v; });
  const int n = (Tb - 1 + 63) / 64, t0 = 1 + lane * n, t1 = t0 + n < Tb ? t0 + n : Tb;
  float psi = lane == 0 ? r0 : CTC_NEG;
  for (int t = t0; t < t1; ++t) psi = lse2(psi, phi[t] + yc[t]);
#pragma unroll
  for (int o = 32; o; o >>= 1) psi = lse2(psi, __shfl_xor(psi, o, 64));
  __syncthreads();
  // r_b(t,h) = lse(r_b(t-1,h) + y_t(blank), r_n(t-1,h) + y_t(blank)) from r_b(0,h) = log 0
  if (lane == 0) so[0] = make_float2(r0, CTC_NEG);
  wave_recurrence(Tb, CTC_NEG, [&](int t) { return yb[t]; }, [&](int t) { return rn[t - 1] + yb[t]; },
                  [&](int t, float v) { so[t] = make_float2(rn[t], v); });
  if (lane == 0) {
    p.psi_out[bk] = floor_neg(psi);
    p.last_out[bk] = c;
  }
}

int prefix_lds(size_t bytes, const char *what) {
  const int have = device_lds_bytes();
  const size_t limit = have > 0 && have < 160 * 1024 ? (size_t)have : (size_t)160 * 1024;
  if (bytes > limit)
    return fail(NABU_EUNSUP, "%s: needs %zu bytes of LDS, a workgroup has %zu here (fewer frames)", what, bytes, limit);
  return 0;
}
int prefix_dims(int B, int W, int T, int C, const char *what) {
  if (B <= 0 || W <= 0 || T <= 0 || C <= 1) return fail(NABU_EINVAL, "%s: bad dimensions", what);
  if ((long long)B * W > (1 << 20)) return fail(NABU_EUNSUP, "%s: B*beam_width too large", what);
  return 0;
}
}  // namespace

// the three steps for beam_run (decode.hip) and the entry points below
int ctc_prefix_lds_ok(int T) { return prefix_lds(4 * (size_t)T * sizeof(float), "ctc_prefix"); }

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_ctc_prefix_prepare(int B, int W, int T, int C, const float *logits, const int32_t *enc_len,
                                       float *norm, float *state, float *psi, int32_t *last, nabu_stream_t stream) {
  NABU_TRY(prefix_dims(B, W, T, C, "ctc_prefix_prepare"));
  NABU_CHECK_ARG(logits && enc_len && norm && state && psi && last, "ctc_prefix_prepare: null pointer");
  const size_t lds = (size_t)T * sizeof(float);
  NABU_TRY(prefix_lds(lds, "ctc_prefix_prepare"));
  PrefixArgs a = {};
  a.B = B; a.W = W; a.T = T; a.C = C; a.logits = logits; a.enc_len = enc_len; a.norm = norm;
  a.state_out = state; a.psi_out = psi; a.last_out = last;
  return launch_lds(ctc_prefix_prepare_kernel, dim3(B), dim3(256), lds, static_cast<hipStream_t>(stream), a);
}

extern "C" int nabu_ctc_prefix_score(int B, int W, int T, int C, const float *logits, const int32_t *enc_len,
                                     const float *norm, const float *state, const float *psi, const int32_t *last,
                                     const int32_t *finished, float *delta, nabu_stream_t stream) {
  NABU_TRY(prefix_dims(B, W, T, C, "ctc_prefix_score"));
  NABU_CHECK_ARG(logits && enc_len && norm && state && psi && last && finished && delta, "ctc_prefix_score: null pointer");
  const size_t lds = 4 * (size_t)T * sizeof(float);
  NABU_TRY(prefix_lds(lds, "ctc_prefix_score"));
  PrefixArgs a = {};
  a.B = B; a.W = W; a.T = T; a.C = C; a.logits = logits; a.enc_len = enc_len; a.norm = const_cast<float *>(norm);
  a.state_in = state; a.psi_in = psi; a.last_in = last; a.finished = finished; a.delta = delta;
  const int threads = C <= 64 ? 64 : (C <= 128 ? 128 : 256);
  return launch_lds(ctc_prefix_score_kernel, dim3(B * W), dim3(threads), lds, static_cast<hipStream_t>(stream), a);
}

extern "C" int nabu_ctc_prefix_advance(int B, int W, int T, int C, const float *logits, const int32_t *enc_len,
                                       const float *norm, const float *state_in, const float *psi_in,
                                       const int32_t *last_in, const int32_t *parent, const int32_t *stay,
                                       const int32_t *pred, float *state_out, float *psi_out, int32_t *last_out,
                                       nabu_stream_t stream) {
  NABU_TRY(prefix_dims(B, W, T, C, "ctc_prefix_advance"));
  NABU_CHECK_ARG(logits && enc_len && norm && state_in && psi_in && last_in && parent && stay && pred && state_out &&
                 psi_out && last_out, "ctc_prefix_advance: null pointer");
  NABU_CHECK_ARG(state_in != state_out && psi_in != psi_out && last_in != last_out,
                 "ctc_prefix_advance: the new state must not overwrite the old one");
  const size_t lds = 4 * (size_t)T * sizeof(float);
  NABU_TRY(prefix_lds(lds, "ctc_prefix_advance"));
  PrefixArgs a = {};
  a.B = B; a.W = W; a.T = T; a.C = C; a.logits = logits; a.enc_len = enc_len; a.norm = const_cast<float *>(norm);
  a.state_in = state_in; a.psi_in = psi_in; a.last_in = last_in; a.parent = parent; a.stay = stay; a.pred = pred;
  a.state_out = state_out; a.psi_out = psi_out; a.last_out = last_out;
  return launch_lds(ctc_prefix_advance_kernel, dim3(B * W), dim3(64), lds, static_cast<hipStream_t>(stream), a);
}
