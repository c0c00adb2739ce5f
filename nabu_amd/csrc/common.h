// common.h — shared helpers of libnabu_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/nabu_hip.h"

namespace nabu {

// thread-local last-error text returned by nabu_last_error()
char *err_buf();
int fail(int code, const char *fmt, ...);

#define NABU_CHECK_ARG(cond, ...)                          \
  do {                                                     \
    if (!(cond)) return ::nabu::fail(NABU_EINVAL, __VA_ARGS__); \
  } while (0)

#define NABU_HIP(call)                                                        \
  do {                                                                        \
    hipError_t e_ = (call);                                                   \
    if (e_ != hipSuccess)                                                     \
      return ::nabu::fail((int)e_, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define NABU_LAUNCH_CHECK()                                                   \
  do {                                                                        \
    hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess)                                                     \
      return ::nabu::fail((int)e_, "kernel launch failed (%s:%d): %s", __FILE__, \
                          __LINE__, hipGetErrorString(e_));                   \
  } while (0)

// a call that reports its own error: pass it on
#define NABU_TRY(call) do { int e_ = (call); if (e_) return e_; } while (0)

// ---- launching a kernel with a large dynamic-LDS request (common.hip) --------------------------------------------------
// Makes sure `fn` may be launched with `bytes` of dynamic LDS on the CURRENT device.  Up to 64 KiB is the runtime's default
// and needs nothing; up to 160 KiB (what a CU has) hipFuncAttributeMaxDynamicSharedMemorySize is raised; more is
// NABU_EUNSUP.  The attribute belongs to the function object on a device, not to the calling thread, so the largest size
// granted per (function, device) is kept in ONE process-wide table behind a mutex and only ever grows: a later, smaller
// request (of any thread) finds the grant and leaves it alone.  A request that finds no room in the table sets the
// attribute on every call.
int ensure_dynamic_lds(const void *fn, size_t bytes);
template <typename K, typename... Args>
static inline int launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
  if (int e = ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), lds)) return e;
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  NABU_LAUNCH_CHECK();
  return 0;
}
// compute units of the CURRENT device as the runtime reports them (partitioned / CPX modes expose fewer than the 256 of a
// whole MI355X), and the LDS a workgroup may use there (the runtime reports it under one of three attribute names
// depending on its version: the largest answer).  Cached per thread and device; 0: the query failed
int device_cus();
int device_lds_bytes();
// the runtime's occupancy answer for (fn, threads, lds) on the current device, the LDS request granted first; cached
int max_blocks_per_cu(const void *fn, int threads, size_t lds, int *blocks);
// Launch of a kernel whose workgroups poll each other, so that co-residency of the whole grid is a REQUIREMENT: the grid
// is validated against the occupancy answer before it is launched — what hipLaunchCooperativeKernel would check,
// without its +15-19 us per launch.  admit(blocks_per_cu) is the caller's rule: 0, or the error it reports.
// dry: validate only (every chunk of a call is validated before the first one is enqueued)
template <typename K, typename A, typename Admit>
static inline int launch_coresident(K kernel, const A &args, int grid, int threads, size_t lds, Admit admit,
                                    hipStream_t stream, bool dry) {
  int blocks = 0;
  if (int e = max_blocks_per_cu(reinterpret_cast<const void *>(kernel), threads, lds, &blocks)) return e;
  if (int e = admit(blocks)) return e;
  if (dry) return 0;
  return launch_lds(kernel, dim3(grid), dim3(threads), lds, stream, args);
}
// an integer environment switch, read on every call (a site that reads its switch once keeps the result in a static)
int env_int(const char *name, int dflt);

// C = op(A)·op(B) (+ beta*C) (+ bias) on row-major operands (the Speller's drivers and the beam search)
static inline int mm(bool ta, bool tb, int M, int N, int K, const float *A, int lda, const float *Bm, int ldb, float beta,
                     float *C, int ldc, const float *bias, float *ws, size_t wsb, nabu_stream_t st) {
  return nabu_gemm_f32(ta, tb, M, N, K, 1.f, A, lda, Bm, ldb, beta, C, ldc, bias, 0, 0, 0, ws, wsb, st);
}

// speller.hip: x[r*ld] = 1 for r < rows (initial alignments of the windowed attention)
int first_col_one(int rows, int ld, float *x, hipStream_t s);

// elementwise.hip: dropout / scheduled sampling on a sub-batch of rows with the whole batch's random stream
int dropout_rows(size_t n, const float *x, float *y, float keep_prob, unsigned long long seed, unsigned long long offset,
                 size_t first_elem, hipStream_t stream);
// one decoder step's scheduled sampling in one launch ([h | ctx] . Wout + bias evaluated only for the rows that are
// sampled): elementwise.hip, sample_step_kernel
bool sample_step_ok(int C);
int sample_step(int B, int C, int U, int E, const float *h, int ldh, const float *ctx, int ldc, const float *Wout,
                const float *bias, float prob, unsigned long long seed, unsigned long long offset, const int32_t *teacher_ids,
                int32_t *out_ids, int b0, hipStream_t stream);
int sample_ids_rows(int B, int C, const float *logits, float prob, unsigned long long seed, unsigned long long offset,
                    const int32_t *teacher_ids, int32_t *out_ids, int b0, hipStream_t stream);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// elementwise.hip: up to 8 regions set to a 32-bit pattern each — or, a region with `from`, copied from a kept array of
// the same length — by ONE launch (ptr 16-byte aligned, a whole number of 4-byte words).  Stands where a layer call
// needs several hipMemsetAsync in a row — exchange rings (0xFF), row-maximum arrays (0 or an a-priori bound): every
// memset is its own dispatch and costs ~6 us of queue gap behind a kernel.
// elementwise.hip: out0[c] = sum_r part[r * ld + c], out1[c] = sum_r part[r * ld + N + c] for a FEW rows (the per-unit
// bias-gradient partials of the persistent backward kernel, both cells): one launch, fixed order
int colsum_pair(int rows, int N, const float *part, int ld, float *out0, float *out1, hipStream_t stream);
// (from: the region is a COPY of `words` words found there — a kept array moved into place by the same launch — not `value`)
struct FillSeg { void *ptr; size_t words; unsigned value; const void *from = nullptr; };
int multi_fill(const FillSeg *segs, int n, hipStream_t stream);

// wave64 reductions through the lane exchange; every lane gets the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// wave_max written out.  The compiler schedules the two forms differently: the softmax kernels of speller.hip were
// tuned with this one and keep it
__device__ __forceinline__ float wave_max_unrolled(float v) {
  v = fmaxf(v, __shfl_xor(v, 32)); v = fmaxf(v, __shfl_xor(v, 16)); v = fmaxf(v, __shfl_xor(v, 8));
  v = fmaxf(v, __shfl_xor(v, 4)); v = fmaxf(v, __shfl_xor(v, 2)); v = fmaxf(v, __shfl_xor(v, 1));
  return v;
}

// block-wide arg-max of the selection kernels (decode.hip, transducer_beam.hip): W rounds of block_best take the W
// best of the candidates the threads hold
struct Best {
  float v;
  int i;
};
// larger value wins, equal values go to the smaller index; NaN never wins
__device__ __forceinline__ Best better(Best a, Best b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// NT threads per workgroup.  `red` holds two sets of NT / 64 per-wave results used alternately (parity = round & 1), so
// that one barrier per round suffices: round k+1 writes the other set while stragglers still read set k.
template <int NT>
__device__ __forceinline__ Best block_best(Best x, Best *red, int parity) {
  red += parity * (NT / 64);
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    Best y;
    y.v = __shfl_xor(x.v, o);
    y.i = __shfl_xor(x.i, o);
    x = better(x, y);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  Best r = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) r = better(r, red[w]);
  return r;
}

// relu that keeps NaN (fmaxf returns the non-NaN operand: a diverged pre-activation would become an ordinary zero and the
// layer norm behind it finite numbers); every other value is fmaxf(x, 0)'s, bit for bit
__device__ __forceinline__ float relu_value(float x) { return x != x ? x : fmaxf(x, 0.f); }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
// tanh through one exp: 2*sigmoid(2x)-1 (abs error ~1e-7)
__device__ __forceinline__ float tanhf_(float x) { return 2.0f / (1.0f + __expf(-2.0f * x)) - 1.0f; }

// counter-based RNG (Philox4x32-10) for dropout masks, scheduled sampling and Gaussian input noise:
// element i uses counter (i/4, offset) and key seed, so the backward pass
// regenerates the forward mask instead of storing it.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // (one 32 x 32 -> 64 multiply per product — v_mad_u64_u32 — instead of a high and a low one: the multiplies run at
    //  a quarter of the vector rate and are what a dropout pass is bound by)
    const unsigned long long p0 = (unsigned long long)M0 * c.x, p1 = (unsigned long long)M1 * c.z;
    const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0;
    const unsigned hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }
// One draw from Categorical(softmax(l[0..C))) by the inverse CDF in class order, u in [0, 1): ONE thread walks the row,
// so the order of every sum is fixed.  The walk of nabu_sample_ids, the step chain's sample_step and nabu_sample_advance
// — the same logits and the same u give the same class in all three, bit for bit.
__device__ __forceinline__ int softmax_draw(const float *l, int C, float u) {
  float m = l[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  float tot = 0.f;
  for (int c = 0; c < C; ++c) tot += expf(l[c] - m);
  const float target = u * tot;        // inverse CDF of softmax(l)
  float acc = 0.f;
  for (int c = 0; c < C; ++c) {
    acc += expf(l[c] - m);
    if (acc > target) return c;
  }
  return C - 1;
}
// dropout scale factors (0 or 1/keep) of the 4-element group `group` of the array the stream is defined on
// (dropout_kernel of elementwise.hip: element e = 4 group + j keeps its value when u01(r[j]) < keep)
__device__ __forceinline__ float4 dropout_scale4(unsigned long long group, float keep, unsigned long long seed,
                                                 unsigned long long offset) {
  const uint4 r = philox4x32_10(make_uint4((unsigned)group, (unsigned)(group >> 32), (unsigned)offset, (unsigned)(offset >> 32)),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  const float inv = 1.0f / keep;
  return make_float4(u01(r.x) < keep ? inv : 0.f, u01(r.y) < keep ? inv : 0.f, u01(r.z) < keep ? inv : 0.f,
                     u01(r.w) < keep ? inv : 0.f);
}
// the four standard normal values of the 4-element group `group` of the array the stream is defined on: Box-Muller on
// (0,1] uniforms, element 4 group + j takes lane j (gaussian_noise_kernel and weight_noise_kernel of elementwise.hip,
// oracle/philox.py: gaussian)
__device__ __forceinline__ float4 gaussian4(unsigned long long group, unsigned long long seed, unsigned long long offset) {
  const uint4 r = philox4x32_10(make_uint4((unsigned)group, (unsigned)(group >> 32), (unsigned)offset, (unsigned)(offset >> 32)),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  const float u1 = 1.0f - u01(r.x), u2 = u01(r.y), u3 = 1.0f - u01(r.z), u4 = u01(r.w);
  const float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
  float sa, ca, sb, cb;
  sincosf(6.283185307179586f * u2, &sa, &ca);
  sincosf(6.283185307179586f * u4, &sb, &cb);
  return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

}  // namespace nabu
