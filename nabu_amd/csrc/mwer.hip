// mwer.hip — minimum word error rate training of the Speller (Prabhavalkar et al. 2018) on the device:
//   nabu_mwer_prepare       beams of the attention beam search -> stacked teacher-forcing targets, slot-major
//   nabu_rows_tile_f32      y[r*B + b, :] = x[b, :]             (one encoder pass under R = N + 1 decoder rows)
//   nabu_rows_tile_bwd_f32  dx[b, :] = sum_r dy[r*B + b, :]     (fixed order r = 0..R-1)
//   nabu_mwer_loss_grad     softmax over the valid hypotheses, expected errors, reference cross-entropy and the gradient
//                           with respect to every logit, in ONE launch
//
// The loss kernel's layout is xent_kernel's (ctc.hip): one workgroup per utterance, one thread per frame, here over the
// (N + 1) * L frames of the utterance's N hypothesis rows and its reference row.
//   pass 1   every frame's log-normaliser lz and its term lz - x[y]
//   between  nll_n: one wave per slot sums the slot's terms (lane-strided partials in time order, then the xor butterfly);
//            then lane n of the first wave walks the N slots in order: maximum, posterior, centred weights, risk
//   pass 2   dlogits = coefficient of the slot * (exp(x - lz) - onehot), zeros where the contract says zero
// No atomics, and every sum has one order: two calls give the same bits.
//
// Where the per-frame words live between the passes: in LDS while 2 * (N + 1) * L floats fit into 48 KiB (every Speller
// recipe: cfg3 needs 1.8 KiB), otherwise in words 0 and 1 of the frame's own dlogits row (C >= 2), which pass 2
// overwrites after the frame's thread has read them back.  The second route was chosen over recomputing (a third read
// of the logits and a second pair of transcendental loops per frame) and over a caller's workspace (an argument, a size
// function and an allocation for an array that fits into memory the call owns anyway): there is no nabu_mwer_ws_bytes.
#include <float.h>

#include "common.h"

namespace nabu {

constexpr int MWER_MAX_N = 16;
constexpr int MWER_T = 256;
constexpr size_t MWER_LDS_MAX = 48 * 1024;     // (the kernel's static words come on top; the default limit is 64 KiB)

// ---------------------------------------------------------------------------
// One workgroup per utterance.  Slot n is valid when its score is a real one and no lower slot with a real score holds
// the same labels [:length] (the lengths do not count the end label, so an unfinished "a b" and a finished
// "a b <end>" compare equal).  Invalid rows get the target [<end>] of length 1.
__global__ __launch_bounds__(64) void mwer_prepare_kernel(int B, int N, int S, int lds, int C,
                                                          const int32_t *__restrict__ sequences,
                                                          const int32_t *__restrict__ lengths,
                                                          const float *__restrict__ scores, int ldr,
                                                          const int32_t *__restrict__ targets,
                                                          const int32_t *__restrict__ target_len, int ldt,
                                                          int32_t *__restrict__ stk_targets, int32_t *__restrict__ stk_len,
                                                          int32_t *__restrict__ hyp_len, int32_t *__restrict__ valid) {
  __shared__ int s_len[MWER_MAX_N], s_real[MWER_MAX_N], s_ok[MWER_MAX_N];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < N) {
    s_len[tid] = min(max(lengths[(size_t)b * N + tid], 0), S);
    s_real[tid] = scores[(size_t)b * N + tid] > -1e30f;            // (false for NaN)
  }
  __syncthreads();
  if (tid < N) {
    const int len = s_len[tid];
    const int32_t *mine = sequences + ((size_t)b * N + tid) * lds;
    int ok = s_real[tid];
    for (int m = 0; m < tid && ok; ++m) {
      if (!s_real[m] || s_len[m] != len) continue;
      const int32_t *other = sequences + ((size_t)b * N + m) * lds;
      int same = 1;
      for (int j = 0; j < len; ++j) same &= mine[j] == other[j];
      if (same) ok = 0;
    }
    s_ok[tid] = ok;
  }
  __syncthreads();
  for (int n = 0; n < N; ++n) {
    const size_t row = (size_t)n * B + b;
    const int ok = s_ok[n], len = ok ? s_len[n] : 0;
    const int32_t *src = sequences + ((size_t)b * N + n) * lds;
    for (int j = tid; j < ldt; j += 64) stk_targets[row * ldt + j] = j < len ? src[j] : (j == len ? C - 1 : 0);
    if (tid == 0) {
      stk_len[row] = len + 1;
      hyp_len[row] = len;
      valid[row] = ok;
    }
  }
  const size_t row = (size_t)N * B + b;
  const int tl = min(max(target_len[b], 0), min(ldr, ldt));
  for (int j = tid; j < ldt; j += 64) stk_targets[row * ldt + j] = j < tl ? targets[(size_t)b * ldr + j] : 0;
  if (tid == 0) stk_len[row] = tl;
}

// ---------------------------------------------------------------------------
// Tiling.  x is n = B * F contiguous floats and y / dy hold R copies of that extent, so the kernels see flat arrays.  A
// thread owns four consecutive elements that start on a 16-byte boundary of x (dx): it moves them as one float4 on
// that side, and on the other side (whose phase changes from replica to replica when n % 4 != 0) as a float4 where the
// address is aligned and as four words where it is not.  The elements in front of the first boundary and behind the
// last whole group go one by one.
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
__global__ __launch_bounds__(256) void rows_tile_kernel(int R, size_t n, size_t head, const float *__restrict__ src,
                                                        float *__restrict__ dst) {
  // !BWD: src = x [n], dst = y [R, n];  BWD: src = dy [R, n], dst = dx [n]
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = head + 4 * g;
  if (g == 0) {
    for (size_t j = 0; j < head; ++j) {
      if (BWD) {
        float acc = src[j];
        for (int r = 1; r < R; ++r) acc += src[(size_t)r * n + j];
        dst[j] = acc;
      } else {
        const float v = src[j];
        for (int r = 0; r < R; ++r) dst[(size_t)r * n + j] = v;
      }
    }
  }
  if (i >= n) return;
  if (i + 4 <= n) {
    if (BWD) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int r = 0; r < R; ++r) {
        const float *p = src + (size_t)r * n + i;
        float4 v;
        if (aligned16(p)) v = *reinterpret_cast<const float4 *>(p);
        else v = make_float4(p[0], p[1], p[2], p[3]);
        if (r == 0) acc = v;
        else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
      }
      *reinterpret_cast<float4 *>(dst + i) = acc;
    } else {
      const float4 v = *reinterpret_cast<const float4 *>(src + i);
      for (int r = 0; r < R; ++r) {
        float *p = dst + (size_t)r * n + i;
        if (aligned16(p)) *reinterpret_cast<float4 *>(p) = v;
        else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
      }
    }
    return;
  }
  for (size_t j = i; j < n; ++j) {
    if (BWD) {
      float acc = src[j];
      for (int r = 1; r < R; ++r) acc += src[(size_t)r * n + j];
      dst[j] = acc;
    } else {
      const float v = src[j];
      for (int r = 0; r < R; ++r) dst[(size_t)r * n + j] = v;
    }
  }
}

template <bool BWD>
static int rows_tile_launch(const char *what, int R, int B, int F, const float *src, float *dst, nabu_stream_t stream) {
  if (!(R > 0 && B > 0 && F > 0)) return fail(NABU_EINVAL, "%s: bad dimensions", what);
  if (!(src && dst)) return fail(NABU_EINVAL, "%s: null pointer", what);
  const float *one = BWD ? dst : src;                            // the side that holds one copy decides the groups
  if (reinterpret_cast<uintptr_t>(one) & 3) return fail(NABU_EINVAL, "%s: operand not aligned to 4 bytes", what);
  const size_t n = (size_t)B * F;
  size_t head = ((16 - (reinterpret_cast<uintptr_t>(one) & 15)) & 15) / 4;
  if (head > n) head = n;
  const size_t groups = (n - head + 3) / 4;
  const size_t blocks = groups ? (groups + 255) / 256 : 1;       // (thread 0 of block 0 moves the head)
  if (blocks > 0x7fffffffu) return fail(NABU_EUNSUP, "%s: %zu elements are more than one launch takes", what, n);
  hipLaunchKernelGGL(rows_tile_kernel<BWD>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), R, n,
                     head, src, dst);
  NABU_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
struct MwerArgs {
  int B, N, L, C, ldt;
  const float *logits;
  const int32_t *targets, *len, *errors, *valid;
  float ce_weight, grad_scale;
  float *loss, *risk, *nll_ref, *dlogits;
};

// IN_LDS: the per-frame words (lz, term) live in dsm[f] and dsm[F + f]; otherwise in words 0 and 1 of the frame's
// dlogits row
template <bool IN_LDS>
__global__ __launch_bounds__(MWER_T) void mwer_kernel(MwerArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  __shared__ float s_nll[MWER_MAX_N + 1], s_coef[MWER_MAX_N + 1];
  const int b = blockIdx.x, tid = threadIdx.x, B = p.B, N = p.N, L = p.L, C = p.C;
  const int F = (N + 1) * L;
  auto lz_at = [&](int f) -> float & {
    if (IN_LDS) return dsm[f];
    return p.dlogits[((size_t)((f / L) * B + b) * L + f % L) * C];
  };
  auto term_at = [&](int f) -> float & {
    if (IN_LDS) return dsm[F + f];
    return p.dlogits[((size_t)((f / L) * B + b) * L + f % L) * C + 1];
  };
  // ---- pass 1
  for (int f = tid; f < F; f += MWER_T) {
    const int n = f / L, t = f - n * L;
    const size_t r = (size_t)n * B + b;
    const int len = min(max(p.len[r], 0), L);
    const bool used = n == N || p.valid[r] != 0;
    float lz = 0.f, term = 0.f;
    if (used && t < len) {
      const float *x = p.logits + (r * L + t) * C;
      float m = x[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
      float z = 0.f;
      for (int c = 0; c < C; ++c) z += expf(x[c] - m);
      lz = m + logf(z);
      const int y = min(max(p.targets[r * p.ldt + t], 0), C - 1);
      term = lz - x[y];
    }
    lz_at(f) = lz;
    term_at(f) = term;
  }
  __syncthreads();
  // ---- nll per slot: wave w takes slots w, w + 4, ...
  for (int n = tid >> 6; n <= N; n += MWER_T / 64) {
    float acc = 0.f;
    for (int t = tid & 63; t < L; t += 64) acc += term_at(n * L + t);
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_nll[n] = acc;
  }
  __syncthreads();
  // ---- posterior over the valid slots, centred weights, risk: lane n walks all slots in order
  if (tid < N) {
    const int *err = p.errors, *val = p.valid;
    float mx = -INFINITY;
    for (int m = 0; m < N; ++m)
      if (val[(size_t)m * B + b]) mx = fmaxf(mx, -s_nll[m]);
    float den = 0.f;
    for (int m = 0; m < N; ++m)
      if (val[(size_t)m * B + b]) den += expf(-s_nll[m] - mx);
    const int e_n = err[(size_t)tid * B + b];
    float centred = 0.f, risk = 0.f;
    for (int m = 0; m < N; ++m) {
      if (!val[(size_t)m * B + b]) continue;
      const float pm = expf(-s_nll[m] - mx) / den;
      const int e_m = err[(size_t)m * B + b];
      centred += pm * (float)(e_n - e_m);            // (equal counts: every term is 0, whatever pm)
      risk += pm * (float)e_m;
    }
    const float pn = val[(size_t)tid * B + b] ? expf(-s_nll[tid] - mx) / den : 0.f;
    s_coef[tid] = val[(size_t)tid * B + b] ? -p.grad_scale * (pn * centred) : 0.f;
    if (tid == 0) {
      const float ref = s_nll[N];
      p.risk[b] = risk;
      p.nll_ref[b] = ref;
      p.loss[b] = p.ce_weight == 0.f ? risk : risk + p.ce_weight * ref;
      s_coef[N] = p.ce_weight * p.grad_scale;
    }
  }
  __syncthreads();
  // ---- pass 2
  for (int f = tid; f < F; f += MWER_T) {
    const int n = f / L, t = f - n * L;
    const size_t r = (size_t)n * B + b;
    const int len = min(max(p.len[r], 0), L);
    const float coef = s_coef[n], lz = lz_at(f);
    float *d = p.dlogits + (r * L + t) * C;
    if (t >= len || coef == 0.f) {                     // (a NaN coefficient is not 0: it reaches the gradient)
      for (int c = 0; c < C; ++c) d[c] = 0.f;
      continue;
    }
    const float *x = p.logits + (r * L + t) * C;
    const int y = min(max(p.targets[r * p.ldt + t], 0), C - 1);
    for (int c = 0; c < C; ++c) d[c] = coef * (expf(x[c] - lz) - (c == y ? 1.f : 0.f));
  }
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_mwer_prepare(int B, int N, int S, int lds, int C, const int32_t *sequences, const int32_t *lengths,
                                 const float *scores, int ldr, const int32_t *targets, const int32_t *target_len, int ldt,
                                 int32_t *stk_targets, int32_t *stk_len, int32_t *hyp_len, int32_t *valid,
                                 nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && N > 0 && S >= 0 && lds >= S && C > 1 && ldr > 0 && ldt > S, "mwer_prepare: bad dimensions");
  NABU_CHECK_ARG((sequences || S == 0) && lengths && scores && targets && target_len && stk_targets && stk_len && hyp_len &&
                     valid, "mwer_prepare: null pointer");
  if (N > MWER_MAX_N) return fail(NABU_EUNSUP, "mwer_prepare: N=%d hypotheses, at most %d", N, MWER_MAX_N);
  hipLaunchKernelGGL(mwer_prepare_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), B, N, S, lds, C,
                     sequences, lengths, scores, ldr, targets, target_len, ldt, stk_targets, stk_len, hyp_len, valid);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_rows_tile_f32(int R, int B, int F, const float *x, float *y, nabu_stream_t stream) {
  return rows_tile_launch<false>("rows_tile", R, B, F, x, y, stream);
}

extern "C" int nabu_rows_tile_bwd_f32(int R, int B, int F, const float *dy, float *dx, nabu_stream_t stream) {
  return rows_tile_launch<true>("rows_tile_bwd", R, B, F, dy, dx, stream);
}

extern "C" int nabu_mwer_loss_grad(int B, int N, int L, int C, int ldt, const float *logits, const int32_t *stk_targets,
                                   const int32_t *stk_len, const int32_t *errors, const int32_t *valid, float ce_weight,
                                   float grad_scale, float *loss, float *risk, float *nll_ref, float *dlogits,
                                   nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && N > 0 && L > 0 && C > 0 && ldt >= L, "mwer_loss_grad: bad dimensions");
  NABU_CHECK_ARG(logits && stk_targets && stk_len && errors && valid && loss && risk && nll_ref && dlogits,
                 "mwer_loss_grad: null pointer");
  NABU_CHECK_ARG(ce_weight >= 0.f && ce_weight <= FLT_MAX, "mwer_loss_grad: ce_weight must be finite and >= 0");  // (false for NaN)
  NABU_CHECK_ARG(fabsf(grad_scale) <= FLT_MAX, "mwer_loss_grad: grad_scale must be finite");
  if (N > MWER_MAX_N) return fail(NABU_EUNSUP, "mwer_loss_grad: N=%d hypotheses, at most %d", N, MWER_MAX_N);
  if (C < 2 || C > 1023)
    return fail(NABU_EUNSUP, "mwer_loss_grad: C=%d classes, 2..1023 are supported (the wide-class kernels have no Speller)", C);
  if ((size_t)(N + 1) * L > 0x3fffffffu) return fail(NABU_EUNSUP, "mwer_loss_grad: L=%d is more than one workgroup walks", L);
  MwerArgs p;
  p.B = B; p.N = N; p.L = L; p.C = C; p.ldt = ldt;
  p.logits = logits; p.targets = stk_targets; p.len = stk_len; p.errors = errors; p.valid = valid;
  p.ce_weight = ce_weight; p.grad_scale = grad_scale;
  p.loss = loss; p.risk = risk; p.nll_ref = nll_ref; p.dlogits = dlogits;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t lds = 2 * (size_t)(N + 1) * L * sizeof(float);
  if (lds <= MWER_LDS_MAX) return launch_lds(mwer_kernel<true>, dim3(B), dim3(MWER_T), lds, s, p);
  return launch_lds(mwer_kernel<false>, dim3(B), dim3(MWER_T), 0, s, p);
}
