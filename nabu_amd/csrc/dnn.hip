// dnn.hip — the frame-level kernels of the DNN encoder and the Kaldi-hybrid recipe (DNN/WSJ of the reference):
// splice + stack, unstack and its adjoint, fused per-frame ReLU + layer norm both ways, the wide-class softmax
// cross-entropy and the log-softmax-minus-prior of the AlignmentDecoder.  All fp32, deterministic (no float atomics).
// Row work is one wave64 per row; rows of the stacked matrices are found from the length vector on the device
// (the exclusive scan of len[0..b) is summed by each workgroup: B is a batch size, a few dozen entries).
#include <algorithm>

#include "common.h"

namespace nabu {

namespace {

constexpr int DNN_LN_MAX_F = 4096;          // fused relu+layer-norm: F <= 64 lanes x 16 float4
constexpr int DNN_LN_VEC = DNN_LN_MAX_F / 256;
constexpr int DNN_LN_BWD_PARTS = 1024;      // waves (= partial rows of dgamma/dbeta) of the backward kernel

__device__ __forceinline__ int clamp_len(int v, int hi) { return min(max(v, 0), hi); }

// exclusive scan of len[0..b) (clamped to [0, T]), the first row of utterance b in the stacked matrix
__device__ __forceinline__ long long row_offset(const int32_t *__restrict__ len, int b, int T) {
  long long off = 0;
  for (int i = 0; i < b; ++i) off += clamp_len(len[i], T);
  return off;
}

// ---------------------------------------------------------------------------------------------- splice + stack
// out[off_b + t, j*F + f] = x[b, t + s_j, f] if 0 <= t + s_j < T else 0, for t < len[b]; s = 0, +1, -1, +2, -2, ...
// out[r, c'F .. ld) = 0.  One wave per output row, four consecutive columns per lane (ld % 4 == 0: 16-byte stores).
__global__ __launch_bounds__(256) void splice_stack_kernel(int B, int T, int F, int context, int ld,
                                                           const float *__restrict__ x, const int32_t *__restrict__ len,
                                                           float *__restrict__ out) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int n = clamp_len(len[b], T);
  if (t >= n) return;
  const long long r = row_offset(len, b, T) + t;
  const int K = (2 * context - 1) * F;
  float *o = out + r * ld;
  for (int c0 = lane * 4; c0 < ld; c0 += 256) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      float val = 0.f;
      if (c < K) {
        const int j = c / F, f = c - j * F;
        const int s = j == 0 ? 0 : ((j & 1) ? (j + 1) >> 1 : -(j >> 1));
        const int ts = t + s;
        if (ts >= 0 && ts < T) val = x[((size_t)b * T + ts) * F + f];
      }
      v[k] = val;
    }
    *reinterpret_cast<float4 *>(o + c0) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ------------------------------------------------------------------------------------- unstack / stack of rows
// UNSTACK: out[b, t, :] = rows[off_b + t, :] for t < len[b], 0 for len[b] <= t < Tm.
// STACK (the adjoint): rows[off_b + t, :] = g[b, t, :] for t < len[b].   One wave per frame.
template <bool UNSTACK, bool VEC>
__global__ __launch_bounds__(256) void rows_move_kernel(int B, int Tm, int H, const int32_t *__restrict__ len,
                                                        const float *__restrict__ src, float *__restrict__ dst) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= Tm) return;
  const int n = clamp_len(len[b], Tm);
  if (!UNSTACK && t >= n) return;
  const size_t frame = ((size_t)b * Tm + t) * H;
  const size_t row = t < n ? (size_t)(row_offset(len, b, Tm) + t) * H : 0;
  const float *s = UNSTACK ? src + row : src + frame;
  float *d = UNSTACK ? dst + frame : dst + row;
  const bool live = t < n;
  if (VEC) {
    for (int c = lane * 4; c < H; c += 256)
      *reinterpret_cast<float4 *>(d + c) = live ? *reinterpret_cast<const float4 *>(s + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int c = lane; c < H; c += 64) d[c] = live ? s[c] : 0.f;
  }
}

// ------------------------------------------------------------------------------ fused ReLU + per-row layer norm
// r = max(z, 0); mean, var over the F entries of the row; y = (r - mean) * rstd * gamma + beta, rstd = 1/sqrt(var+eps).
// One wave per row, the row held in registers (lane owns float4 i*64 + lane, i < F/256 rounded up).
__global__ __launch_bounds__(256) void relu_ln_fwd_kernel(int N, int F, const float *__restrict__ z,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          float eps, float *__restrict__ y, float *__restrict__ mean,
                                                          float *__restrict__ rstd) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const int F4 = F >> 2;
  const float4 *zr = reinterpret_cast<const float4 *>(z + (size_t)row * F);
  float4 v[DNN_LN_VEC];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < DNN_LN_VEC; ++i) {
    const int q = i * 64 + lane;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < F4) {
      const float4 a = zr[q];
      v[i] = make_float4(relu_value(a.x), relu_value(a.y), relu_value(a.z), relu_value(a.w));
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  // (divisions, not a reciprocal: the mean of a constant row is then exact and its variance zero)
  const float fF = (float)F;
  const float mu = wave_sum(s) / fF;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < DNN_LN_VEC; ++i) {
    if (i * 64 + lane < F4) {
      const float a = v[i].x - mu, b_ = v[i].y - mu, c = v[i].z - mu, d = v[i].w - mu;
      ss += (a * a + b_ * b_) + (c * c + d * d);
    }
  }
  const float rs = 1.0f / sqrtf(wave_sum(ss) / fF + eps);
  float4 *yr = reinterpret_cast<float4 *>(y + (size_t)row * F);
  const float4 *g4 = reinterpret_cast<const float4 *>(gamma);
  const float4 *b4 = reinterpret_cast<const float4 *>(beta);
#pragma unroll
  for (int i = 0; i < DNN_LN_VEC; ++i) {
    const int q = i * 64 + lane;
    if (q < F4) {
      const float4 g = g4[q], bb = b4[q];
      yr[q] = make_float4((v[i].x - mu) * rs * g.x + bb.x, (v[i].y - mu) * rs * g.y + bb.y,
                          (v[i].z - mu) * rs * g.z + bb.z, (v[i].w - mu) * rs * g.w + bb.w);
    }
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// Backward: xhat = (relu(z) - mean) * rstd, g = dy * gamma,
//   dr = rstd * (g - mean_F(g) - xhat * mean_F(g * xhat)),  dz = z > 0 ? dr : 0;
// wave w of P takes rows w, w + P, ... and sums dy * xhat and dy over them in that order: partial row w of
// dgamma_part / dbeta_part [P, F] (reduced by nabu_colsum_f32).  One wave per workgroup.
__global__ __launch_bounds__(64) void relu_ln_bwd_kernel(int N, int F, const float *__restrict__ z,
                                                         const float *__restrict__ dy, const float *__restrict__ gamma,
                                                         const float *__restrict__ mean, const float *__restrict__ rstd,
                                                         float *__restrict__ dz, float *__restrict__ dgp,
                                                         float *__restrict__ dbp) {
  const int lane = threadIdx.x;
  const int P = gridDim.x;
  const int F4 = F >> 2;
  const float4 *g4 = reinterpret_cast<const float4 *>(gamma);
  float4 ag[DNN_LN_VEC], ab[DNN_LN_VEC];
#pragma unroll
  for (int i = 0; i < DNN_LN_VEC; ++i) ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float fF = (float)F;
  for (int row = blockIdx.x; row < N; row += P) {
    const float4 *zr = reinterpret_cast<const float4 *>(z + (size_t)row * F);
    const float4 *dr = reinterpret_cast<const float4 *>(dy + (size_t)row * F);
    const float mu = mean[row], rs = rstd[row];
    float4 zv[DNN_LN_VEC], gv[DNN_LN_VEC];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < DNN_LN_VEC; ++i) {
      const int q = i * 64 + lane;
      zv[i] = gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < F4) {
        zv[i] = zr[q];
        const float4 d = dr[q], g = g4[q];
        const float4 xh = make_float4((relu_value(zv[i].x) - mu) * rs, (relu_value(zv[i].y) - mu) * rs,
                                      (relu_value(zv[i].z) - mu) * rs, (relu_value(zv[i].w) - mu) * rs);
        ag[i].x += d.x * xh.x; ag[i].y += d.y * xh.y; ag[i].z += d.z * xh.z; ag[i].w += d.w * xh.w;
        ab[i].x += d.x; ab[i].y += d.y; ab[i].z += d.z; ab[i].w += d.w;
        gv[i] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
        s1 += (gv[i].x + gv[i].y) + (gv[i].z + gv[i].w);
        s2 += (gv[i].x * xh.x + gv[i].y * xh.y) + (gv[i].z * xh.z + gv[i].w * xh.w);
      }
    }
    const float m1 = wave_sum(s1) / fF, m2 = wave_sum(s2) / fF;
    float4 *o = reinterpret_cast<float4 *>(dz + (size_t)row * F);
#pragma unroll
    for (int i = 0; i < DNN_LN_VEC; ++i) {
      const int q = i * 64 + lane;
      if (q < F4) {
        const float4 a = zv[i], g = gv[i];
        float4 r;
        r.x = a.x > 0.f ? rs * (g.x - m1 - (a.x - mu) * rs * m2) : 0.f;
        r.y = a.y > 0.f ? rs * (g.y - m1 - (a.y - mu) * rs * m2) : 0.f;
        r.z = a.z > 0.f ? rs * (g.z - m1 - (a.z - mu) * rs * m2) : 0.f;
        r.w = a.w > 0.f ? rs * (g.w - m1 - (a.w - mu) * rs * m2) : 0.f;
        o[q] = r;
      }
    }
  }
  float4 *pg = reinterpret_cast<float4 *>(dgp + (size_t)blockIdx.x * F);
  float4 *pb = reinterpret_cast<float4 *>(dbp + (size_t)blockIdx.x * F);
#pragma unroll
  for (int i = 0; i < DNN_LN_VEC; ++i) {
    const int q = i * 64 + lane;
    if (q < F4) {
      pg[q] = ag[i];
      pb[q] = ab[i];
    }
  }
}

// ------------------------------------------------------------------------------------------ wide-class rows
// One wave per frame row of C logits: pass 1 = online max / sum-exp over the row (head to 16-byte alignment, float4
// body, scalar tail), pass 2 re-reads the row (still in cache) and writes the output row.
//   XENT: out = grad_scale / target_len[b] * (softmax - onehot(y)); term[b*L+t] = logsumexp - x[y]
//   XENT, SMOOTH: the target is q = (1 - smoothing) * onehot(y) + smoothing / C: out = scale * (softmax - q),
//     term = logsumexp - (1 - smoothing) * x[y] - smoothing * mean(x); the row sum is taken in pass 1, from the values
//     that pass loads anyway.  The term is summed as (1 - smoothing) * (lz - x[y]) + smoothing * (lz - mean(x)) and
//     the gradient as (softmax - smoothing / C) - (1 - smoothing) * [c = y], as in xent_kernel.  SMOOTH = false is
//     the expression order the kernel always had.
//   PRIOR: out = x - logsumexp - logprior
// Rows t >= len[b] are written as zeros (term 0).
struct OnlineLse {
  float m, s;
  __device__ __forceinline__ void add(float x) {
    if (x > m) {
      s = s * expf(m - x) + 1.f;
      m = x;
    } else {
      s += expf(x - m);
    }
  }
  __device__ __forceinline__ void add4(float4 v) {
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    const float nm = fmaxf(m, mx);
    s = s * expf(m - nm) + ((expf(v.x - nm) + expf(v.y - nm)) + (expf(v.z - nm) + expf(v.w - nm)));
    m = nm;
  }
};

template <bool XENT, bool VEC, bool SMOOTH = false>
__global__ __launch_bounds__(256) void wide_rows_kernel(int B, int L, int C, int ldt, const float *__restrict__ logits,
                                                        const int32_t *__restrict__ targets,
                                                        const int32_t *__restrict__ len,
                                                        const int32_t *__restrict__ target_len, float grad_scale,
                                                        float smoothing, const float *__restrict__ logprior,
                                                        float *__restrict__ term,
                                                        float *__restrict__ out) {
  const size_t frame = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (frame >= (size_t)B * L) return;
  const int b = (int)(frame / L), t = (int)(frame - (size_t)b * L);
  const float *x = logits + frame * C;
  float *o = out + frame * C;
  // elements before the first 16-byte boundary of the row, and the float4 body after them
  const int head = VEC ? min((int)((4 - ((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3), C) : C;
  const int body4 = VEC ? (C - head) >> 2 : 0;
  const int tail0 = head + 4 * body4;
  if (t >= clamp_len(len[b], L)) {
    for (int c = lane; c < head; c += 64) o[c] = 0.f;
    float4 *o4 = reinterpret_cast<float4 *>(o + head);
    for (int q = lane; q < body4; q += 64) o4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = tail0 + lane; c < C; c += 64) o[c] = 0.f;
    if (XENT && lane == 0) term[frame] = 0.f;
    return;
  }
  OnlineLse acc{-INFINITY, 0.f};
  float sx = 0.f;                                  // SMOOTH: this lane's part of the row sum
  for (int c = lane; c < head; c += 64) {
    const float v = x[c];
    acc.add(v);
    if (SMOOTH) sx += v;
  }
  const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
  for (int q = lane; q < body4; q += 64) {
    const float4 v = x4[q];
    acc.add4(v);
    if (SMOOTH) sx += (v.x + v.y) + (v.z + v.w);
  }
  for (int c = tail0 + lane; c < C; c += 64) {
    const float v = x[c];
    acc.add(v);
    if (SMOOTH) sx += v;
  }
  const float m = wave_max(acc.m);
  const float s = wave_sum(acc.s == 0.f ? 0.f : acc.s * expf(acc.m - m));
  const float lz = m + logf(s);
  if (XENT) {
    const int y = targets[(size_t)b * ldt + t];
    const float scale = grad_scale / (float)target_len[b];
    const float keep = 1.0f - smoothing, spread = smoothing / (float)C;      // SMOOTH: q = keep * onehot + spread
    const float mean = SMOOTH ? wave_sum(sx) / (float)C : 0.f;
    // (a label outside [0, C) is not read: its term is NaN, as the reference's op would fail on it)
    if (lane == 0) {
      float v = __int_as_float(0x7fc00000);
      if ((unsigned)y < (unsigned)C) v = SMOOTH ? keep * (lz - x[y]) + smoothing * (lz - mean) : lz - x[y];
      term[frame] = v;
    }
    auto grad = [&](float v, int c) {
      return SMOOTH ? scale * ((expf(v - lz) - spread) - (c == y ? keep : 0.f))
                    : scale * (expf(v - lz) - (c == y ? 1.f : 0.f));
    };
    for (int c = lane; c < head; c += 64) o[c] = grad(x[c], c);
    float4 *o4 = reinterpret_cast<float4 *>(o + head);
    for (int q = lane; q < body4; q += 64) {
      const float4 v = x4[q];
      const int c = head + 4 * q;
      o4[q] = make_float4(grad(v.x, c), grad(v.y, c + 1), grad(v.z, c + 2), grad(v.w, c + 3));
    }
    for (int c = tail0 + lane; c < C; c += 64) o[c] = grad(x[c], c);
  } else {
    for (int c = lane; c < head; c += 64) o[c] = x[c] - lz - logprior[c];
    float4 *o4 = reinterpret_cast<float4 *>(o + head);
    for (int q = lane; q < body4; q += 64) {
      const float4 v = x4[q];
      const int c = head + 4 * q;
      // logprior is read with scalar loads: its alignment relative to the row is arbitrary
      o4[q] = make_float4(v.x - lz - logprior[c], v.y - lz - logprior[c + 1], v.z - lz - logprior[c + 2],
                          v.w - lz - logprior[c + 3]);
    }
    for (int c = tail0 + lane; c < C; c += 64) o[c] = x[c] - lz - logprior[c];
  }
}

// loss[b] = (sum_{t<L} term[b*L + t]) / target_len[b], fixed-order: thread k sums t = k, k+256, ..., then a tree
__global__ __launch_bounds__(256) void wide_loss_sum_kernel(int L, const float *__restrict__ term,
                                                            const int32_t *__restrict__ target_len,
                                                            float *__restrict__ loss) {
  __shared__ float red[256];
  const int b = blockIdx.x;
  float acc = 0.f;
  for (int t = threadIdx.x; t < L; t += 256) acc += term[(size_t)b * L + t];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[b] = red[0] / (float)target_len[b];
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace nabu

using namespace nabu;

extern "C" int nabu_splice_stack_f32(int B, int T, int F, int context, const float *x, const int32_t *len,
                                     float *out, int ld, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && F > 0 && context >= 1, "splice_stack: bad dimensions");
  NABU_CHECK_ARG((long long)(2 * context - 1) * F <= ld && ld % 4 == 0, "splice_stack: ld must be >= (2c-1)F and a multiple of 4");
  NABU_CHECK_ARG(x && len && out, "splice_stack: null pointer");
  NABU_CHECK_ARG(aligned16(out), "splice_stack: out must be 16-byte aligned");
  hipLaunchKernelGGL(splice_stack_kernel, dim3((T + 3) / 4, B), dim3(256), 0, static_cast<hipStream_t>(stream), B, T,
                     F, context, ld, x, len, out);
  NABU_LAUNCH_CHECK();
  return 0;
}

static int rows_move(bool unstack, int B, int Tm, int H, const int32_t *len, const float *src, float *dst,
                     nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && Tm >= 0 && H > 0, "unstack/stack rows: bad dimensions");
  if (Tm == 0) return 0;
  NABU_CHECK_ARG(len && src && dst, "unstack/stack rows: null pointer");
  const bool vec = H % 4 == 0 && aligned16(src) && aligned16(dst);
  const dim3 grid((Tm + 3) / 4, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (unstack) {
    if (vec) hipLaunchKernelGGL((rows_move_kernel<true, true>), grid, dim3(256), 0, s, B, Tm, H, len, src, dst);
    else hipLaunchKernelGGL((rows_move_kernel<true, false>), grid, dim3(256), 0, s, B, Tm, H, len, src, dst);
  } else {
    if (vec) hipLaunchKernelGGL((rows_move_kernel<false, true>), grid, dim3(256), 0, s, B, Tm, H, len, src, dst);
    else hipLaunchKernelGGL((rows_move_kernel<false, false>), grid, dim3(256), 0, s, B, Tm, H, len, src, dst);
  }
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_unstack_rows_f32(int B, int Tm, int H, const int32_t *len, const float *rows, float *out,
                                     nabu_stream_t stream) {
  return rows_move(true, B, Tm, H, len, rows, out, stream);
}

extern "C" int nabu_stack_rows_f32(int B, int Tm, int H, const int32_t *len, const float *g, float *rows,
                                   nabu_stream_t stream) {
  return rows_move(false, B, Tm, H, len, g, rows, stream);
}

static int relu_ln_check(int N, int F) {
  if (F <= 0 || F % 4 != 0 || F > DNN_LN_MAX_F)
    return fail(NABU_EUNSUP, "relu+layer norm: F = %d must be a multiple of 4 and at most %d", F, DNN_LN_MAX_F);
  return N < 0 ? fail(NABU_EINVAL, "relu+layer norm: N < 0") : 0;
}

extern "C" int nabu_rows_relu_ln_fwd(int N, int F, const float *z, const float *gamma, const float *beta, float eps,
                                     float *y, float *mean, float *rstd, nabu_stream_t stream) {
  if (int e = relu_ln_check(N, F)) return e;
  if (N == 0) return 0;
  NABU_CHECK_ARG(z && gamma && beta && y && mean && rstd, "relu+layer norm: null pointer");
  NABU_CHECK_ARG(aligned16(z) && aligned16(gamma) && aligned16(beta) && aligned16(y), "relu+layer norm: unaligned operand");
  hipLaunchKernelGGL(relu_ln_fwd_kernel, dim3((N + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), N, F, z,
                     gamma, beta, eps, y, mean, rstd);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_rows_relu_ln_bwd_parts(int N) { return N <= 0 ? 1 : std::min(N, DNN_LN_BWD_PARTS); }

extern "C" int nabu_rows_relu_ln_bwd(int N, int F, const float *z, const float *dy, const float *gamma,
                                     const float *mean, const float *rstd, float *dz, float *dgamma_part,
                                     float *dbeta_part, nabu_stream_t stream) {
  if (int e = relu_ln_check(N, F)) return e;
  NABU_CHECK_ARG(dgamma_part && dbeta_part && aligned16(dgamma_part) && aligned16(dbeta_part),
                 "relu+layer norm bwd: null or unaligned partials");
  const int P = nabu_rows_relu_ln_bwd_parts(N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (N == 0) {
    NABU_HIP(hipMemsetAsync(dgamma_part, 0, (size_t)F * sizeof(float), s));
    NABU_HIP(hipMemsetAsync(dbeta_part, 0, (size_t)F * sizeof(float), s));
    return 0;
  }
  NABU_CHECK_ARG(z && dy && gamma && mean && rstd && dz, "relu+layer norm bwd: null pointer");
  NABU_CHECK_ARG(aligned16(z) && aligned16(dy) && aligned16(gamma) && aligned16(dz), "relu+layer norm bwd: unaligned operand");
  hipLaunchKernelGGL(relu_ln_bwd_kernel, dim3(P), dim3(64), 0, s, N, F, z, dy, gamma, mean, rstd, dz, dgamma_part,
                     dbeta_part);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t nabu_xent_wide_ws_bytes(int B, int L) {
  if (B <= 0 || L <= 0) return 0;
  return (size_t)B * L * sizeof(float);
}

static int xent_wide_launch(int B, int L, int C, int ldt, const float *logits, const int32_t *targets,
                            const int32_t *logit_len, const int32_t *target_len, float grad_scale, float smoothing,
                            float *loss, float *dlogits, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && L > 0 && C > 0 && ldt >= L, "xent_wide: bad dimensions");
  NABU_CHECK_ARG(logits && targets && logit_len && target_len && loss && dlogits && ws, "xent_wide: null pointer");
  NABU_CHECK_ARG(smoothing >= 0.f && smoothing < 1.f, "xent_wide: smoothing must be in [0, 1)");      // (false for NaN)
  const size_t need = nabu_xent_wide_ws_bytes(B, L);
  if (ws_bytes < need) return fail(NABU_EWS, "xent_wide: workspace %zu < %zu", ws_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *term = static_cast<float *>(ws);
  const size_t frames = (size_t)B * L;
  const dim3 grid((unsigned)((frames + 3) / 4));
  // the float4 body needs logits and dlogits equally placed against a 16-byte boundary
  const bool vec = ((reinterpret_cast<uintptr_t>(logits) ^ reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
  auto kern = smoothing > 0.f ? (vec ? wide_rows_kernel<true, true, true> : wide_rows_kernel<true, false, true>)
                              : (vec ? wide_rows_kernel<true, true> : wide_rows_kernel<true, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, B, L, C, ldt, logits, targets, logit_len, target_len, grad_scale,
                     smoothing, nullptr, term, dlogits);
  NABU_LAUNCH_CHECK();
  hipLaunchKernelGGL(wide_loss_sum_kernel, dim3(B), dim3(256), 0, s, L, term, target_len, loss);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_xent_wide_loss_grad(int B, int L, int C, int ldt, const float *logits, const int32_t *targets,
                                        const int32_t *logit_len, const int32_t *target_len, float grad_scale,
                                        float *loss, float *dlogits, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return xent_wide_launch(B, L, C, ldt, logits, targets, logit_len, target_len, grad_scale, 0.f, loss, dlogits, ws,
                          ws_bytes, stream);
}

extern "C" int nabu_xent_wide_smooth_loss_grad(int B, int L, int C, int ldt, const float *logits,
                                               const int32_t *targets, const int32_t *logit_len,
                                               const int32_t *target_len, float grad_scale, float smoothing,
                                               float *loss, float *dlogits, void *ws, size_t ws_bytes,
                                               nabu_stream_t stream) {
  return xent_wide_launch(B, L, C, ldt, logits, targets, logit_len, target_len, grad_scale, smoothing, loss, dlogits,
                          ws, ws_bytes, stream);
}

extern "C" int nabu_log_softmax_prior_f32(int B, int T, int C, const float *x, const int32_t *len,
                                          const float *logprior, float *out, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T >= 0 && C > 0, "log_softmax_prior: bad dimensions");
  if (T == 0) return 0;
  NABU_CHECK_ARG(x && len && logprior && out, "log_softmax_prior: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(((size_t)B * T + 3) / 4));
  if (((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(out)) & 15) == 0)
    hipLaunchKernelGGL((wide_rows_kernel<false, true>), grid, dim3(256), 0, s, B, T, C, T, x, nullptr, len, nullptr,
                       0.f, 0.f, logprior, nullptr, out);
  else
    hipLaunchKernelGGL((wide_rows_kernel<false, false>), grid, dim3(256), 0, s, B, T, C, T, x, nullptr, len, nullptr,
                       0.f, 0.f, logprior, nullptr, out);
  NABU_LAUNCH_CHECK();
  return 0;
}
