// elementwise.hip — HBM-bound helpers: fused clip+Adam, bias-gradient column
// sums, time padding for odd-length pyramid stacks.
#include <float.h>

#include "common.h"

namespace nabu {

// tf.clip_by_value propagates NaN (min/max of the TF kernels are plain comparisons), fminf/fmaxf
// return the non-NaN operand: a diverged gradient must stay visible, not become -clip.
__device__ __forceinline__ float clip_value(float x, float clip) {
  return x != x ? x : fminf(fmaxf(x, -clip), clip);
}

// ---------------------------------------------------------------------------
// fused clip + TF-style Adam: 4 streams read (param, grad, m, v), 3 written.
// 16-byte accesses, grid-stride, 7*4 = 28 algorithmic bytes per parameter.
struct AdamHyper {
  float lr_t, b1, b2, eps;
};

// rn(a * b) as a value of its own.  Under -ffp-contract=fast the backend fuses any product into a sum it feeds, whatever the
// source says (`#pragma clang fp contract(off)` is disregarded in that mode, and __fmul_rn is a plain product here); a
// value that has passed an asm statement is no product to it.  The statement emits no instruction.
__device__ __forceinline__ float rounded_product(float a, float b) {
  float ab = a * b;
  asm("" : "+v"(ab));
  return ab;
}

// The Adam update of one element on the gradient x, every rounding of m and v written down: the bits of a training
// trajectory must not depend on which product a compiler chooses to contract.
// FUSED (the 16-byte groups, which is all a training buffer has: Variables.flatten pads every variable to a multiple of
// 4): one rounding each for b1 m + ((1 - b1) x) and for x ((1 - b2) x) + (b2 v).
// !FUSED (the n % 4 elements after them, which only tests reach): every product and sum rounded.  The form exists only to
// keep the bits this tail has always had.
// lr_t m / (sqrt(v) + eps) has no product feeding a sum, so nothing there can be contracted.
// tests/test_hip_update_bits.py holds both forms to bits recorded on the device.
template <bool FUSED>
__device__ __forceinline__ void adam1(float &p, float &m, float &v, float x, const AdamHyper &h) {
  if (FUSED) {
    m = fmaf(h.b1, m, (1.f - h.b1) * x);
    v = fmaf(x, (1.f - h.b2) * x, h.b2 * v);
  } else {
    m = rounded_product(h.b1, m) + rounded_product(1.f - h.b1, x);
    v = rounded_product(h.b2, v) + rounded_product((1.f - h.b2) * x, x);
  }
  p -= h.lr_t * m / (sqrtf(v) + h.eps);
}

// the gradient adam_kernel's update takes, from the last micro-batch's g and the sum `a` of the earlier ones (ACC)
template <bool ACC, bool NORM>
__device__ __forceinline__ float adam_gradient(float a, float g, float gscale, float clip) {
  if (NORM) return (ACC ? a + g : g) * gscale;
  return clip_value((ACC ? a + clip_value(g, clip) : g) * gscale, clip);
}

// FROM: the parameter is read from `src` instead of p (the update of a step whose forward and backward passes ran at
// p = src + noise).
// ACC: the gradient is the sum of `acc`, an update's earlier micro-batch gradients, and g, the last one: one more stream
// read, 32 bytes per parameter, and no accumulate pass before the update.
// NORM false: clipping by value.  x = clamp((ACC ? acc + clamp(g) : g) * gscale), both clamps to +-clip.
// NORM true: clipping by the global norm (nabu_grad_norm_f32 ran before on the same stream).  x = (ACC ? acc + g : g) *
// stats[1], read on the device, no clamp; clip and gscale are not read.  A NaN factor is a skipped update: m and v are
// not touched and the parameter is not updated — with FROM p still becomes src, because it holds the noisy values of a
// weight-noise step at this point.  Bit for bit the NORM = false kernel at clip = +inf and gscale = stats[1].
template <bool FROM, bool ACC, bool NORM>
__global__ __launch_bounds__(256) void adam_kernel(size_t n, float *__restrict__ p, const float *__restrict__ src,
                                                   const float *__restrict__ acc, const float *__restrict__ g,
                                                   float *__restrict__ m, float *__restrict__ v, AdamHyper h, float clip,
                                                   float gscale, const float *__restrict__ stats) {
  if (NORM) gscale = stats[1];
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (NORM && gscale != gscale) {
    if (FROM) {
      for (size_t i = tid; i < n4; i += stride) reinterpret_cast<float4 *>(p)[i] = reinterpret_cast<const float4 *>(src)[i];
      for (size_t i = n4 * 4 + tid; i < n; i += stride) p[i] = src[i];
    }
    return;
  }
  for (size_t i = tid; i < n4; i += stride) {
    float4 pp = FROM ? reinterpret_cast<const float4 *>(src)[i] : reinterpret_cast<float4 *>(p)[i];
    const float4 gg = reinterpret_cast<const float4 *>(g)[i];
    const float4 aa = ACC ? reinterpret_cast<const float4 *>(acc)[i] : float4{};
    float4 mm = reinterpret_cast<float4 *>(m)[i];
    float4 vv = reinterpret_cast<float4 *>(v)[i];
    adam1<true>(pp.x, mm.x, vv.x, adam_gradient<ACC, NORM>(aa.x, gg.x, gscale, clip), h);
    adam1<true>(pp.y, mm.y, vv.y, adam_gradient<ACC, NORM>(aa.y, gg.y, gscale, clip), h);
    adam1<true>(pp.z, mm.z, vv.z, adam_gradient<ACC, NORM>(aa.z, gg.z, gscale, clip), h);
    adam1<true>(pp.w, mm.w, vv.w, adam_gradient<ACC, NORM>(aa.w, gg.w, gscale, clip), h);
    reinterpret_cast<float4 *>(p)[i] = pp;
    reinterpret_cast<float4 *>(m)[i] = mm;
    reinterpret_cast<float4 *>(v)[i] = vv;
  }
  for (size_t i = n4 * 4 + tid; i < n; i += stride) {
    float pp = FROM ? src[i] : p[i], mm = m[i], vv = v[i];
    adam1<false>(pp, mm, vv, adam_gradient<ACC, NORM>(ACC ? acc[i] : 0.f, g[i], gscale, clip), h);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
}

// out = clamp(g, +-clip) (+ acc): one micro-batch's clipped gradient added to the sum of the earlier ones.  ACC false is
// the first micro-batch: a pure write, the accumulator is neither cleared nor read (8 bytes per parameter, 12 with acc).
// out may BE acc or g (no __restrict__: every thread reads its elements before it writes them, nobody else touches them);
// ACC false with out = g is the clamp in place of nabu_clip_f32.
template <bool ACC>
__global__ __launch_bounds__(256) void clip_accumulate_kernel(size_t n, float *out, const float *acc, const float *g,
                                                              float clip) {
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n4; i += stride) {
    float4 x = reinterpret_cast<const float4 *>(g)[i];
    x.x = clip_value(x.x, clip);
    x.y = clip_value(x.y, clip);
    x.z = clip_value(x.z, clip);
    x.w = clip_value(x.w, clip);
    if (ACC) {
      const float4 a = reinterpret_cast<const float4 *>(acc)[i];
      x.x += a.x;
      x.y += a.y;
      x.z += a.z;
      x.w += a.w;
    }
    reinterpret_cast<float4 *>(out)[i] = x;
  }
  for (size_t i = n4 * 4 + tid; i < n; i += stride) {
    const float x = clip_value(g[i], clip);
    out[i] = ACC ? x + acc[i] : x;
  }
}

// ---------------------------------------------------------------------------
// global-norm clipping (the [trainer] key clip_gradient_norm): the L2 norm of the flat gradient in two launches, and the
// Adam update that reads its scale factor from the device (adam_kernel with NORM).
// block-wide sum of one double (fixed tree: deterministic); the result is red[0]
__device__ __forceinline__ void block_sum_f64(double s, double *red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

// stage 1: partial[block] = sum of x^2 over the block's grid-stride share, x = g or (fp32) acc + g, what
// adam_kernel forms with NORM.  A product of two floats is exact in double and every term is >= 0, so the sum carries a
// relative error of (additions in the longest chain) * 2^-53 whatever the magnitudes: 1e30 does not overflow, 1e-30 does
// not vanish.  4 or 8 bytes read per parameter; the conversions and double FMAs are far below the vector rate.  A thread
// keeps one chain per lane of its 16-byte groups and joins them in a fixed order.
template <bool ACC>
__global__ __launch_bounds__(256) void grad_norm_stage1(size_t n, const float *__restrict__ g,
                                                        const float *__restrict__ acc, double *__restrict__ partial) {
  __shared__ double red[256];
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  // (two groups per iteration, twice the bytes in flight, measured no faster: 29.8 against 30.4 us over cfg2's buffer)
  for (size_t i = tid; i < n4; i += stride) {
    float4 x = reinterpret_cast<const float4 *>(g)[i];
    if (ACC) {
      const float4 a = reinterpret_cast<const float4 *>(acc)[i];
      x.x = a.x + x.x;
      x.y = a.y + x.y;
      x.z = a.z + x.z;
      x.w = a.w + x.w;
    }
    s0 = fma((double)x.x, (double)x.x, s0);
    s1 = fma((double)x.y, (double)x.y, s1);
    s2 = fma((double)x.z, (double)x.z, s2);
    s3 = fma((double)x.w, (double)x.w, s3);
  }
  double s = (s0 + s1) + (s2 + s3);
  for (size_t i = n4 * 4 + tid; i < n; i += stride) {      // (n % 4 elements: threads 0..2 of block 0)
    const float x = ACC ? acc[i] + g[i] : g[i];
    s = fma((double)x, (double)x, s);
  }
  block_sum_f64(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// stage 2, one block behind a kernel boundary (the partials of other XCDs are visible): S = sum of the partials in a
// fixed order, then the four words of `stats`.  norm = (float)(scale * sqrt(S)); factor = what the update multiplies the
// gradient sum by: scale, times max_norm / norm when the norm exceeds max_norm (a norm of 0 never divides); a norm that
// is NaN or inf gives factor = NaN, which adam_kernel takes as "skip", and counts in stats[2].
__global__ __launch_bounds__(256) void grad_norm_stage2(int nparts, const double *__restrict__ partial, float scale,
                                                        float max_norm, float *__restrict__ stats) {
  __shared__ double red[256];
  double s = 0.0;
  for (int p = threadIdx.x; p < nparts; p += 256) s += partial[p];
  block_sum_f64(s, red);
  if (threadIdx.x != 0) return;
  const float norm = (float)((double)scale * sqrt(red[0]));
  const bool finite = fabsf(norm) <= FLT_MAX;               // (false for NaN)
  const float factor = norm > max_norm ? scale * (max_norm / norm) : scale;
  int32_t *words = reinterpret_cast<int32_t *>(stats);
  stats[0] = norm;
  stats[1] = finite ? factor : __int_as_float(0x7fc00000);
  if (!finite) words[2] += 1;
  words[3] = 0;
}

// ---------------------------------------------------------------------------
// column sums: stage 1 -> partial[rs][N], stage 2 -> out[N].  Fixed summation
// order => bitwise reproducible bias gradients.
constexpr int CS_ROWS = 512;  // rows per stage-1 block

__global__ __launch_bounds__(256) void colsum_stage1(int M, int N, const float *__restrict__ A,
                                                     int lda, float *__restrict__ partial) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rl = threadIdx.x >> 6;
  const int r0 = blockIdx.y * CS_ROWS;
  const int r1 = min(M, r0 + CS_ROWS);
  float s = 0.f;
  if (c < N)
    for (int r = r0 + rl; r < r1; r += 4) s += A[(size_t)r * lda + c];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < N)
    partial[(size_t)blockIdx.y * N + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) +
                                          (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void colsum_stage2(int nparts, int N,
                                                     const float *__restrict__ partial, float beta,
                                                     float *__restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float s = 0.f;
  for (int p = 0; p < nparts; ++p) s += partial[(size_t)p * N + c];
  out[c] = (beta != 0.f ? beta * out[c] : 0.f) + s;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pad_time_kernel(int B, int T, int Tp, int F,
                                                       const float *__restrict__ x,
                                                       float *__restrict__ y, int unpad) {
  // one thread per float4 (F % 4 == 0 checked by the host) of the larger tensor
  const size_t F4 = F / 4;
  const size_t total = (size_t)B * (unpad ? T : Tp) * F4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t f = i % F4;
    const size_t bt = i / F4;
    const int TT = unpad ? T : Tp;
    const size_t b = bt / TT, t = bt % TT;
    if (unpad) {
      reinterpret_cast<float4 *>(y)[(b * T + t) * F4 + f] =
          reinterpret_cast<const float4 *>(x)[(b * Tp + t) * F4 + f];
    } else {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((int)t < T) v = reinterpret_cast<const float4 *>(x)[(b * T + t) * F4 + f];
      reinterpret_cast<float4 *>(y)[(b * Tp + t) * F4 + f] = v;
    }
  }
}


// counter-based RNG (Philox4x32-10): philox4x32_10 / u01 in common.h (shared with the persistent decoder)

// i0: index of the first 4-element group of x inside the array the random stream is defined on (a
// sub-batch of rows draws exactly the numbers the whole batch would draw for those rows)
__global__ __launch_bounds__(256) void dropout_kernel(size_t n, const float *__restrict__ x,
                                                      float *__restrict__ y, float keep,
                                                      unsigned long long seed, unsigned long long offset, size_t i0) {
  const size_t n4 = (n + 3) / 4;
  const float inv = 1.0f / keep;
  for (size_t il = (size_t)blockIdx.x * 256 + threadIdx.x; il < n4; il += (size_t)gridDim.x * 256) {
    const size_t i = il + i0;
    const uint4 r = philox4x32_10(make_uint4((unsigned)i, (unsigned)(i >> 32), (unsigned)offset,
                                             (unsigned)(offset >> 32)),
                                  make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const unsigned rr[4] = {r.x, r.y, r.z, r.w};
    if (4 * il + 3 < n && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
      // whole group, 16-byte aligned arrays: one load, one store
      const float4 v = *reinterpret_cast<const float4 *>(x + 4 * il);
      *reinterpret_cast<float4 *>(y + 4 * il) = make_float4(u01(rr[0]) < keep ? v.x * inv : 0.f, u01(rr[1]) < keep ? v.y * inv : 0.f,
                                                            u01(rr[2]) < keep ? v.z * inv : 0.f, u01(rr[3]) < keep ? v.w * inv : 0.f);
      continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t e = 4 * il + j;
      if (e < n) y[e] = u01(rr[j]) < keep ? x[e] * inv : 0.f;
    }
  }
}

// scheduled sampling (ScheduledEmbeddingTrainingHelper): one thread per row
__global__ __launch_bounds__(256) void sample_ids_kernel(int B, int C, const float *__restrict__ logits,
                                                         float prob, unsigned long long seed,
                                                         unsigned long long offset,
                                                         const int32_t *__restrict__ teacher,
                                                         int32_t *__restrict__ out, int b0) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint4 r = philox4x32_10(make_uint4((unsigned)(b + b0), 0u, (unsigned)offset, (unsigned)(offset >> 32)),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  int id = teacher[b];
  if (u01(r.x) < prob) id = softmax_draw(logits + (size_t)b * C, C, u01(r.y));
  out[b] = id;
}

// Scheduled sampling of ONE decoder step in ONE launch (the step chain of nabu_speller_fwd): row b draws the Bernoulli of
// sample_ids_kernel first and only a row that IS to be sampled (sample_prob = 0.1 in the reference's defaults: one in
// ten) evaluates its logits [h | ctx] . W_out + b — up to 25 k slots x (C / 4) class quads, 16-byte loads of the weight
// rows — and draws from softmax(logits) by the inverse CDF in class order, exactly as sample_ids_kernel does.  Replaces two
// [Bn, C] products through the general GEMM entry point and the sampling launch per step and sub-batch
// (rnn_decoder.py:59-66, ScheduledEmbeddingTrainingHelper).  Requires C % 4 == 0, C <= 256: the 256 threads hold
// nks = min(25, 256 / (C / 4)) whole k slots (25 up to C = 40, fewer above), slot ks adds k = ks, ks + nks, ... and the
// trailing partial slot of threads (256 % (C / 4) of them) stays idle.
constexpr int SAMPLE_KS = 25;
__global__ __launch_bounds__(256) void sample_step_kernel(int C, int U, int E, const float *__restrict__ h, int ldh,
                                                          const float *__restrict__ ctx, int ldc,
                                                          const float *__restrict__ Wout, const float *__restrict__ bias,
                                                          float prob, unsigned long long seed, unsigned long long offset,
                                                          const int32_t *__restrict__ teacher, int32_t *__restrict__ out, int b0) {
  __shared__ float part[SAMPLE_KS][256];
  __shared__ float lg[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint4 r = philox4x32_10(make_uint4((unsigned)(b + b0), 0u, (unsigned)offset, (unsigned)(offset >> 32)),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  if (!(u01(r.x) < prob)) {
    if (tid == 0) out[b] = teacher[b];
    return;
  }
  const int CQ = C / 4, ks = tid / CQ, cq = tid - ks * CQ, K = U + E, nks = min(SAMPLE_KS, 256 / CQ);
  if (ks < nks) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float *hb = h + (size_t)b * ldh, *cb = ctx + (size_t)b * ldc;
#pragma unroll 8
    for (int k = ks; k < K; k += nks) {
      const float x = k < U ? hb[k] : cb[k - U];
      const float4 wv = *reinterpret_cast<const float4 *>(Wout + (size_t)k * C + 4 * cq);
      acc.x = fmaf(x, wv.x, acc.x); acc.y = fmaf(x, wv.y, acc.y); acc.z = fmaf(x, wv.z, acc.z); acc.w = fmaf(x, wv.w, acc.w);
    }
    *reinterpret_cast<float4 *>(&part[ks][4 * cq]) = acc;
  }
  __syncthreads();
  if (tid < C) {
    float v = bias[tid];
    for (int i = 0; i < nks; ++i) v += part[i][tid];
    lg[tid] = v;
  }
  __syncthreads();
  if (tid == 0) out[b] = softmax_draw(lg, C, u01(r.y));
}

__global__ __launch_bounds__(256) void gaussian_noise_kernel(size_t n, const float *__restrict__ x,
                                                             float *__restrict__ y, float stddev,
                                                             unsigned long long seed,
                                                             unsigned long long offset) {
  const size_t n4 = (n + 3) / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 z4 = gaussian4(i, seed, offset);      // (common.h)
    const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t e = 4 * i + j;
      if (e < n) y[e] = x[e] + stddev * z[j];
    }
  }
}

// Variational weight noise of one training step in ONE launch over the flat parameter buffer (n4 groups of 16 bytes):
// every group is copied to `clean`; a group inside one of the `nranges` sorted, disjoint [first, end) group ranges of
// `ranges` (the matrices: trainer.py, weight_noise_ranges) also becomes p = fmaf(stddev, z, p) in place, with z the
// gaussian4 values of that group of an n-element array, whatever the table.  A group outside every range is not stored to
// p and runs no Philox.  The table is searched from LDS (the last range that starts at or before the group).
constexpr int WN_MAX_RANGES = NABU_WEIGHT_NOISE_MAX_RANGES;
__global__ __launch_bounds__(256) void weight_noise_kernel(size_t n4, float *__restrict__ p, float *__restrict__ clean,
                                                           const int2 *__restrict__ ranges, int nranges, float stddev,
                                                           unsigned long long seed, unsigned long long offset) {
  __shared__ int2 tab[WN_MAX_RANGES];
  for (int k = threadIdx.x; k < nranges; k += 256) tab[k] = ranges[k];
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 v = reinterpret_cast<const float4 *>(p)[i];
    reinterpret_cast<float4 *>(clean)[i] = v;
    const int g = (int)i;                      // (n4 <= INT32_MAX: checked by the host)
    int lo = 0, hi = nranges;                  // lo = number of ranges that start at or before g
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tab[mid].x <= g) lo = mid + 1;
      else hi = mid;
    }
    if (lo == 0 || g >= tab[lo - 1].y) continue;
    const float4 z = gaussian4(i, seed, offset);
    v.x = fmaf(stddev, z.x, v.x);
    v.y = fmaf(stddev, z.y, v.y);
    v.z = fmaf(stddev, z.z, v.z);
    v.w = fmaf(stddev, z.w, v.w);
    reinterpret_cast<float4 *>(p)[i] = v;
  }
}

// out[0] = scale * sum(x[0..n)) — one block, fixed tree (deterministic).
__global__ __launch_bounds__(256) void sum_kernel(size_t n, const float *__restrict__ x, float scale,
                                                  float *__restrict__ out) {
  __shared__ float red[256];
  float s = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 256) s += x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = scale * red[0];
}

__global__ __launch_bounds__(256) void axpy_kernel(size_t n, float a, const float *__restrict__ x,
                                                   float *__restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    y[i] = fmaf(a, x[i], y[i]);
}

__global__ __launch_bounds__(256) void relu_kernel(size_t n, const float *__restrict__ x, float *__restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    y[i] = relu_value(x[i]);
}
__global__ __launch_bounds__(256) void relu_bwd_kernel(size_t n, const float *__restrict__ y,
                                                       const float *__restrict__ dy, float *__restrict__ dx) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// block-wide sums of two values (fixed tree: deterministic)
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red) {
  red[threadIdx.x] = a;
  red[256 + threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x] += red[threadIdx.x + o];
      red[256 + threadIdx.x] += red[256 + threadIdx.x + o];
    }
    __syncthreads();
  }
  a = red[0];
  b = red[256];
  __syncthreads();
}

// one workgroup per batch row; moments over all N = T*F elements of the row
__global__ __launch_bounds__(256) void layer_norm_fwd_kernel(int N, int F, const float *__restrict__ x,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, float eps,
                                                             float *__restrict__ y, float *__restrict__ mean,
                                                             float *__restrict__ rstd) {
  __shared__ float red[512];
  const float *xr = x + (size_t)blockIdx.x * N;
  float *yr = y + (size_t)blockIdx.x * N;
  float s = 0.f, dummy = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) s += xr[i];
  block_sum2(s, dummy, red);
  const float mu = s / N;
  float v = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) { const float d = xr[i] - mu; v = fmaf(d, d, v); }
  block_sum2(v, dummy, red);
  const float rs = rsqrtf(v / N + eps);
  for (int i = threadIdx.x; i < N; i += 256) yr[i] = (xr[i] - mu) * rs * gamma[i % F] + beta[i % F];
  if (threadIdx.x == 0) { mean[blockIdx.x] = mu; rstd[blockIdx.x] = rs; }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)), g = dy*gamma; partial dgamma/dbeta per row
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(int N, int F, const float *__restrict__ x,
                                                             const float *__restrict__ gamma,
                                                             const float *__restrict__ dy,
                                                             const float *__restrict__ mean,
                                                             const float *__restrict__ rstd, float *__restrict__ dx,
                                                             float *__restrict__ dgp, float *__restrict__ dbp) {
  __shared__ float red[512];
  const size_t row = (size_t)blockIdx.x * N;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) {
    const float g = dy[row + i] * gamma[i % F], xh = (x[row + i] - mu) * rs;
    s1 += g;
    s2 = fmaf(g, xh, s2);
  }
  block_sum2(s1, s2, red);
  const float m1 = s1 / N, m2 = s2 / N;
  for (int i = threadIdx.x; i < N; i += 256) {
    const float g = dy[row + i] * gamma[i % F], xh = (x[row + i] - mu) * rs;
    dx[row + i] = rs * (g - m1 - xh * m2);
  }
  // per-feature sums over the row's T frames (thread f walks its column: fixed order)
  for (int f = threadIdx.x; f < F; f += 256) {
    float a = 0.f, b = 0.f;
    for (int i = f; i < N; i += F) {
      const float d = dy[row + i];
      a = fmaf(d, (x[row + i] - mu) * rs, a);
      b += d;
    }
    dgp[(size_t)blockIdx.x * F + f] = a;
    dbp[(size_t)blockIdx.x * F + f] = b;
  }
}

__global__ __launch_bounds__(256) void ceil_div_kernel(int n, const int32_t *__restrict__ in, int d,
                                                       int32_t *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (in[i] + d - 1) / d;
}

__global__ __launch_bounds__(256) void colsum_pair_kernel(int rows, int N, const float *__restrict__ part, int ld,
                                                         float *__restrict__ out0, float *__restrict__ out1) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * N) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += part[(size_t)r * ld + c];
  if (c < N) out0[c] = s;
  else out1[c - N] = s;
}

// several regions, one launch (common.h: multi_fill).  A block covers FILL_CHUNK words of one region.
constexpr int FILL_MAX = 8;
constexpr unsigned FILL_CHUNK = 4096;
struct FillArgs {
  unsigned *ptr[FILL_MAX];
  unsigned long long words[FILL_MAX];
  unsigned value[FILL_MAX];
  const unsigned *from[FILL_MAX];     // non-null: the region is copied from here
  unsigned first_block[FILL_MAX + 1];
  int n;
};
__global__ __launch_bounds__(256) void multi_fill_kernel(FillArgs a) {
  int i = 0;
  while (i + 1 < a.n && blockIdx.x >= a.first_block[i + 1]) ++i;
  const unsigned long long w0 = (unsigned long long)(blockIdx.x - a.first_block[i]) * FILL_CHUNK;
  const unsigned long long w1 = w0 + FILL_CHUNK < a.words[i] ? w0 + FILL_CHUNK : a.words[i];
  const unsigned v = a.value[i];
  unsigned *p = a.ptr[i];
  if (const unsigned *q = a.from[i]) {
    for (unsigned long long w = w0 + threadIdx.x; w < w1; w += 256) p[w] = q[w];
    return;
  }
  for (unsigned long long w = w0 + 4ull * threadIdx.x; w < w1; w += 1024) {
    if (w + 3 < w1) *reinterpret_cast<uint4 *>(p + w) = make_uint4(v, v, v, v);
    else
      for (unsigned long long k = w; k < w1; ++k) p[k] = v;
  }
}

static int grid_for(size_t work_items) {
  size_t b = (work_items + 255) / 256;
  if (b > 2048) b = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace nabu

using namespace nabu;

// true when [a, a + n) and [b, b + n) are the same range or share no element
static bool same_or_disjoint(const float *a, const float *b, size_t n) { return a == b || a + n <= b || b + n <= a; }

// The launch behind the four Adam entry points.  src, acc and stats may be NULL and choose FROM, ACC and NORM; an entry
// point that demands one of them says in `demanded` whether it got it, and reports under its own name `who`.
static int adam_launch(const char *who, bool demanded, size_t n, float *param_out, const float *src, const float *acc,
                       const float *g, float *m, float *v, AdamHyper h, float clip, float gscale, const float *stats,
                       nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(demanded && param_out && g && m && v, "%s: null pointer", who);
  NABU_CHECK_ARG(((uintptr_t)param_out | (uintptr_t)src | (uintptr_t)acc | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v |
                  (uintptr_t)stats) % 16 == 0, "%s: buffers must be 16-byte aligned", who);
  NABU_CHECK_ARG(!src || src + n <= param_out || param_out + n <= src,
                 "%s: src and param_out overlap (the in-place update passes no src)", who);
  NABU_CHECK_ARG(!acc || acc + n <= g || g + n <= acc, "%s: acc and g overlap", who);
  static const decltype(&adam_kernel<false, false, false>) kernels[2][2][2] = {
      {{adam_kernel<false, false, false>, adam_kernel<false, false, true>},
       {adam_kernel<false, true, false>, adam_kernel<false, true, true>}},
      {{adam_kernel<true, false, false>, adam_kernel<true, false, true>},
       {adam_kernel<true, true, false>, adam_kernel<true, true, true>}}};
  hipLaunchKernelGGL(kernels[src != nullptr][acc != nullptr][stats != nullptr], dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, param_out, src, acc, g, m, v, h, clip, gscale, stats);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_adam_clip_step(size_t n, float *param, const float *grad, float *m, float *v,
                                   float lr_t, float b1, float b2, float eps, float clip,
                                   float grad_scale, nabu_stream_t stream) {
  return adam_launch("adam", true, n, param, nullptr, nullptr, grad, m, v, {lr_t, b1, b2, eps}, clip, grad_scale, nullptr,
                     stream);
}

extern "C" int nabu_adam_clip_step_from(size_t n, float *param_out, const float *src, const float *grad, float *m,
                                        float *v, float lr_t, float b1, float b2, float eps, float clip,
                                        float grad_scale, nabu_stream_t stream) {
  return adam_launch("adam_from", src, n, param_out, src, nullptr, grad, m, v, {lr_t, b1, b2, eps}, clip, grad_scale,
                     nullptr, stream);
}

extern "C" int nabu_adam_clip_step_acc(size_t n, float *param_out, const float *src, const float *acc, const float *g,
                                       float *m, float *v, float lr_t, float b1, float b2, float eps, float clip,
                                       float grad_scale, nabu_stream_t stream) {
  return adam_launch("adam_acc", acc, n, param_out, src, acc, g, m, v, {lr_t, b1, b2, eps}, clip, grad_scale, nullptr,
                     stream);
}

extern "C" size_t nabu_grad_norm_ws_bytes(size_t n) { return n ? (size_t)grid_for(n / 4 + 1) * sizeof(double) : 0; }

extern "C" int nabu_grad_norm_f32(size_t n, const float *g, const float *acc, float scale, float max_norm, float *stats,
                                  void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(stats && (n == 0 || g), "grad_norm: null pointer (only acc may be NULL)");
  NABU_CHECK_ARG(((uintptr_t)g | (uintptr_t)acc | (uintptr_t)stats) % 16 == 0 && (uintptr_t)ws % 8 == 0,
                 "grad_norm: g, acc and stats must be 16-byte aligned, the workspace 8-byte aligned");
  NABU_CHECK_ARG(max_norm > 0.f, "grad_norm: max_norm must be > 0");                                       // (false for NaN)
  NABU_CHECK_ARG(scale > 0.f && scale <= FLT_MAX, "grad_norm: scale must be finite and > 0");
  NABU_CHECK_ARG(!acc || !n || acc + n <= g || g + n <= acc, "grad_norm: acc and g overlap");
  const size_t need = nabu_grad_norm_ws_bytes(n);
  if (need && (!ws || ws_bytes < need)) return fail(NABU_EWS, "grad_norm: workspace %zu < %zu", ws_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int parts = (int)(need / sizeof(double));           // a function of n alone: the same n sums in the same order
  if (parts > 0) {
    if (acc)
      hipLaunchKernelGGL(grad_norm_stage1<true>, dim3(parts), dim3(256), 0, s, n, g, acc, static_cast<double *>(ws));
    else
      hipLaunchKernelGGL(grad_norm_stage1<false>, dim3(parts), dim3(256), 0, s, n, g, (const float *)nullptr,
                         static_cast<double *>(ws));
    NABU_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(grad_norm_stage2, dim3(1), dim3(256), 0, s, parts, static_cast<const double *>(ws), scale, max_norm,
                     stats);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_adam_scaled_step(size_t n, float *param_out, const float *src, const float *acc, const float *g,
                                     float *m, float *v, float lr_t, float b1, float b2, float eps, const float *stats,
                                     nabu_stream_t stream) {
  return adam_launch("adam_scaled", stats, n, param_out, src, acc, g, m, v, {lr_t, b1, b2, eps}, 0.f, 0.f, stats, stream);
}

extern "C" int nabu_weight_noise_f32(size_t n, float *param, float *clean, const int32_t *ranges,
                                     const int32_t *ranges_host, int nranges, float stddev, unsigned long long seed,
                                     unsigned long long offset, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(param && clean, "weight_noise: null pointer");
  NABU_CHECK_ARG(n % 4 == 0 && n / 4 <= (size_t)INT32_MAX, "weight_noise: n = %zu must be a multiple of 4 below 2^33", n);
  NABU_CHECK_ARG(((uintptr_t)param | (uintptr_t)clean) % 16 == 0, "weight_noise: buffers must be 16-byte aligned");
  NABU_CHECK_ARG(param + n <= clean || clean + n <= param, "weight_noise: param and clean overlap");
  NABU_CHECK_ARG(stddev >= 0.f && stddev <= FLT_MAX, "weight_noise: stddev must be finite and >= 0");      // (false for NaN)
  NABU_CHECK_ARG(nranges >= 0 && nranges <= WN_MAX_RANGES, "weight_noise: nranges = %d is outside 0..%d", nranges,
                 WN_MAX_RANGES);
  NABU_CHECK_ARG(nranges == 0 || (ranges && ranges_host && (uintptr_t)ranges % 8 == 0),
                 "weight_noise: the range table needs its device copy (8-byte aligned) and its host copy");
  long long prev_end = 0;
  for (int k = 0; k < nranges; ++k) {
    const long long first = ranges_host[2 * k], end = ranges_host[2 * k + 1];
    NABU_CHECK_ARG(first >= prev_end && first < end && end <= (long long)(n / 4),
                   "weight_noise: range %d = [%lld, %lld) is empty, unsorted, overlaps its predecessor or ends past %zu groups",
                   k, first, end, n / 4);
    prev_end = end;
  }
  hipLaunchKernelGGL(weight_noise_kernel, dim3(grid_for(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), n / 4,
                     param, clean, reinterpret_cast<const int2 *>(ranges), nranges, stddev, seed, offset);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_clip_f32(size_t n, float *g, float clip, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(g && (uintptr_t)g % 16 == 0, "clip: null or unaligned pointer");
  hipLaunchKernelGGL(clip_accumulate_kernel<false>, dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, g, (const float *)nullptr, g, clip);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_clip_accumulate_f32(size_t n, float *out, const float *acc, const float *g, float clip,
                                        nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(out && g, "clip_accumulate: null pointer (only acc may be NULL)");
  NABU_CHECK_ARG(((uintptr_t)out | (uintptr_t)acc | (uintptr_t)g) % 16 == 0,
                 "clip_accumulate: buffers must be 16-byte aligned");
  NABU_CHECK_ARG(same_or_disjoint(out, g, n) && (!acc || same_or_disjoint(out, acc, n)),
                 "clip_accumulate: out must be acc, g or a buffer of its own, not a shifted overlap of either");
  if (acc)
    hipLaunchKernelGGL(clip_accumulate_kernel<true>, dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), n, out, acc, g, clip);
  else
    hipLaunchKernelGGL(clip_accumulate_kernel<false>, dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), n, out, (const float *)nullptr, g, clip);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t nabu_colsum_ws_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)((M + CS_ROWS - 1) / CS_ROWS) * N * sizeof(float);
}

extern "C" int nabu_colsum_f32(int M, int N, const float *A, int lda, float beta, float *out,
                               void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(M >= 0 && N > 0 && A && out, "colsum: bad argument");
  const int parts = (M + CS_ROWS - 1) / CS_ROWS;
  const size_t need = (size_t)parts * N * sizeof(float);
  if (parts > 0 && (!ws || ws_bytes < need)) return fail(NABU_EWS, "colsum: workspace %zu < %zu", ws_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (parts > 0) {
    hipLaunchKernelGGL(colsum_stage1, dim3((N + 63) / 64, parts), dim3(256), 0, s, M, N, A, lda,
                       static_cast<float *>(ws));
    NABU_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(colsum_stage2, dim3((N + 255) / 256), dim3(256), 0, s, parts, N,
                     static_cast<const float *>(ws), beta, out);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_pad_time_f32(int B, int T, int Tp, int F, const float *x, float *y,
                                 nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && Tp >= T && F > 0 && F % 4 == 0 && x && y, "pad_time: bad argument");
  hipLaunchKernelGGL(pad_time_kernel, dim3(grid_for((size_t)B * Tp * (F / 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), B, T, Tp, F, x, y, 0);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_unpad_time_f32(int B, int T, int Tp, int F, const float *y, float *x,
                                   nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && Tp >= T && F > 0 && F % 4 == 0 && x && y, "unpad_time: bad argument");
  hipLaunchKernelGGL(pad_time_kernel, dim3(grid_for((size_t)B * T * (F / 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), B, T, Tp, F, y, x, 1);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_dropout_f32(size_t n, const float *x, float *y, float keep_prob,
                                unsigned long long seed, unsigned long long offset,
                                nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(x && y && keep_prob > 0.f && keep_prob <= 1.f, "dropout: bad argument");
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, x, y, keep_prob, seed, offset, (size_t)0);
  NABU_LAUNCH_CHECK();
  return 0;
}

namespace nabu {
int colsum_pair(int rows, int N, const float *part, int ld, float *out0, float *out1, hipStream_t stream) {
  if (rows < 0 || N <= 0 || !part || !out0 || !out1) return fail(NABU_EINVAL, "colsum_pair: bad argument");
  hipLaunchKernelGGL(colsum_pair_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, stream, rows, N, part, ld, out0, out1);
  NABU_LAUNCH_CHECK();
  return 0;
}

int multi_fill(const FillSeg *segs, int n, hipStream_t stream) {
  FillArgs a = {};
  unsigned blocks = 0;
  for (int i = 0; i < n; ++i) {
    if (!segs[i].words) continue;
    if (a.n >= FILL_MAX) return fail(NABU_EINVAL, "multi_fill: more than %d regions", FILL_MAX);
    if (!segs[i].ptr || (reinterpret_cast<uintptr_t>(segs[i].ptr) & 15)) return fail(NABU_EINVAL, "multi_fill: null or unaligned region");
    a.ptr[a.n] = static_cast<unsigned *>(segs[i].ptr);
    a.words[a.n] = segs[i].words;
    a.value[a.n] = segs[i].value;
    a.from[a.n] = static_cast<const unsigned *>(segs[i].from);
    a.first_block[a.n] = blocks;
    blocks += (unsigned)((segs[i].words + FILL_CHUNK - 1) / FILL_CHUNK);
    ++a.n;
  }
  if (!a.n) return 0;
  a.first_block[a.n] = blocks;
  hipLaunchKernelGGL(multi_fill_kernel, dim3(blocks), dim3(256), 0, stream, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

// rows [first_elem, first_elem + n) of a larger array (first_elem % 4 == 0): the same random numbers the
// call on the whole array would use for them
int dropout_rows(size_t n, const float *x, float *y, float keep_prob, unsigned long long seed, unsigned long long offset,
                 size_t first_elem, hipStream_t stream) {
  if (n == 0) return 0;
  // (a start inside a group would read its neighbour's words for the group's other lanes)
  if (first_elem % 4) return fail(NABU_EINVAL, "dropout_rows: first element %zu is not a multiple of 4", first_elem);
  hipLaunchKernelGGL(dropout_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0, stream, n, x, y, keep_prob, seed, offset,
                     first_elem / 4);
  NABU_LAUNCH_CHECK();
  return 0;
}
bool sample_step_ok(int C) { return C % 4 == 0 && C >= 4 && C <= 256; }
int sample_step(int B, int C, int U, int E, const float *h, int ldh, const float *ctx, int ldc, const float *Wout,
                const float *bias, float prob, unsigned long long seed, unsigned long long offset, const int32_t *teacher_ids,
                int32_t *out_ids, int b0, hipStream_t stream) {
  if (B == 0) return 0;
  if (!sample_step_ok(C)) return fail(NABU_EUNSUP, "sample_step: C = %d", C);
  hipLaunchKernelGGL(sample_step_kernel, dim3(B), dim3(256), 0, stream, C, U, E, h, ldh, ctx, ldc, Wout, bias, prob, seed,
                     offset, teacher_ids, out_ids, b0);
  NABU_LAUNCH_CHECK();
  return 0;
}
int sample_ids_rows(int B, int C, const float *logits, float prob, unsigned long long seed, unsigned long long offset,
                    const int32_t *teacher_ids, int32_t *out_ids, int b0, hipStream_t stream) {
  if (B == 0) return 0;
  hipLaunchKernelGGL(sample_ids_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, B, C, logits, prob, seed, offset,
                     teacher_ids, out_ids, b0);
  NABU_LAUNCH_CHECK();
  return 0;
}
}  // namespace nabu

extern "C" int nabu_sample_ids(int B, int C, const float *logits, float prob, unsigned long long seed,
                               unsigned long long offset, const int32_t *teacher_ids, int32_t *out_ids,
                               nabu_stream_t stream) {
  if (B == 0) return 0;
  NABU_CHECK_ARG(B > 0 && C > 0 && logits && teacher_ids && out_ids && prob >= 0.f && prob <= 1.f,
                 "sample_ids: bad argument");
  hipLaunchKernelGGL(sample_ids_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     B, C, logits, prob, seed, offset, teacher_ids, out_ids, 0);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_gaussian_noise_f32(size_t n, const float *x, float *y, float stddev,
                                       unsigned long long seed, unsigned long long offset,
                                       nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(x && y && stddev >= 0.f, "gaussian_noise: bad argument");
  hipLaunchKernelGGL(gaussian_noise_kernel, dim3(grid_for(n / 4 + 1)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), n, x, y, stddev, seed, offset);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_sum_f32(size_t n, const float *x, float scale, float *out, nabu_stream_t stream) {
  NABU_CHECK_ARG(out && (n == 0 || x), "sum: null pointer");
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), n, x, scale, out);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_axpy_f32(size_t n, float a, const float *x, float *y, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(x && y, "axpy: null pointer");
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), n, a, x, y);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_relu_f32(size_t n, const float *x, float *y, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(x && y, "relu: null pointer");
  hipLaunchKernelGGL(relu_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), n, x, y);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_relu_bwd_f32(size_t n, const float *y, const float *dy, float *dx, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(y && dy && dx, "relu_bwd: null pointer");
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), n, y, dy, dx);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_layer_norm_fwd(int B, int N, int F, const float *x, const float *gamma, const float *beta,
                                   float eps, float *y, float *mean, float *rstd, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && N > 0 && F > 0 && N % F == 0 && x && gamma && beta && y && mean && rstd,
                 "layer_norm_fwd: bad argument");
  hipLaunchKernelGGL(layer_norm_fwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), N, F, x, gamma,
                     beta, eps, y, mean, rstd);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_layer_norm_bwd(int B, int N, int F, const float *x, const float *gamma, const float *dy,
                                   const float *mean, const float *rstd, float *dx, float *dgamma_part,
                                   float *dbeta_part, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && N > 0 && F > 0 && N % F == 0 && x && gamma && dy && mean && rstd && dx && dgamma_part &&
                     dbeta_part, "layer_norm_bwd: bad argument");
  hipLaunchKernelGGL(layer_norm_bwd_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), N, F, x, gamma,
                     dy, mean, rstd, dx, dgamma_part, dbeta_part);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_ceil_div_i32(int n, const int32_t *in, int d, int32_t *out, nabu_stream_t stream) {
  if (n == 0) return 0;
  NABU_CHECK_ARG(n > 0 && d > 0 && in && out, "ceil_div: bad argument");
  hipLaunchKernelGGL(ceil_div_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), n, in, d, out);
  NABU_LAUNCH_CHECK();
  return 0;
}
