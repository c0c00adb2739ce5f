// conv_module.hip — the core of the Conformer block's convolution module (Gulati et al. 2020) on a ragged padded batch,
// forward and backward, fp32:
//     g = u[:, :D] . sigmoid(u[:, D:])                 GLU
//     z[t] = bw + sum_k w[k] . g[t + k - (K-1)/2]       depthwise "same" convolution along time, g = 0 outside 0 .. len
//     n = gamma . (z - mean) rstd + beta                layer norm per frame over the D channels
//     y = n . sigmoid(n)                                Swish
// g, z and n never exist in memory.  No matrix instructions: a depthwise convolution reduces over taps only, never over
// channels, so there is no second matrix dimension for an MFMA; the operation is bound by memory and by VALU issue.
//
// FORWARD (cm_fwd_kernel), one launch.  A workgroup of 256 threads owns CM_TT = 32 consecutive frames of one utterance
// and all D channels; z of the tile lives in LDS as [CM_TT][D] (CM_TT D 4 bytes, 128 KiB at D = 1024).
//   Phase 1, thread = channel (chunks of 256 channels).  The thread keeps its taps in registers and slides along the
//   rows + KC - 1 frames of tile and halo: u[t, c] and u[t, D + c] are read coalesced across the wave, g is formed in
//   registers and kept in a KC-deep register window, z goes to LDS.  No halo is stored anywhere.
//     * K becomes a compile-time constant through three zero-padded tap classes KC = 7, 15, 31: the K taps sit centred
//       among KC, the others are 0 (a product with +-0 added to a chain does not change its value).
//     * The window is circular with STATIC indices: the time loop is unrolled over STEPS = KC . RPB frames (28, 30, 31), so
//       frame s lies in register s % KC and no register is ever moved.
//     * Loads are issued LB frames ahead in one batch (addresses clamped into 0 .. len-1, so no branch separates them and
//       no frame at or past len[b] is ever read; the select that zeroes g comes after the load): a thread's walk costs
//       STEPS / LB memory latencies per STEPS frames, not one per frame.
//   Phase 2, wave = frame.  A wave reads its row of z from LDS, takes mean and variance in two passes (a per-lane chain
//   of D / 64 terms, then the fixed wave butterfly), and writes y, mean and rstd.
// BACKWARD, two launches, no float atomics: two calls give equal bits.
//   cm_bwd_norm_kernel has the forward kernel's shape and its phase 1.  Phase 2 recomputes n from z, mean and rstd, forms
//   dn = dy . swish'(n), dz by the layer-norm adjoint (written to the [B,T,D] workspace, the only intermediate in memory,
//   +0.0 at rows >= len) and the workgroup's partial sums of dgamma, dbeta and dbw = sum_t dz: per lane over the wave's
//   frames, then across the four waves through the LDS the z tile no longer needs.
//   cm_bwd_conv_kernel is thread = channel without LDS: a workgroup owns CM_TT frames x 256 channels and slides with two
//   register windows, dz and the recomputed g: dg[t] = sum_k w[k] dz[t - k + (K-1)/2], du from dg, g and sigmoid(u2)
//   (one more exp per output; u2[t] is re-read, a cache hit), and dw[k] += dz[t] g[t + k - (K-1)/2] into KC registers,
//   written as the workgroup's row of partial sums.
// Partial sums are rows [parts, .], parts = nabu_conv_module_parts(B, T); the caller reduces them with nabu_colsum_f32.
// Both sigmoids use the full-precision expf (DESIGN.md section 15 says why).  Built with packed fp32 VALU instructions
// switched off (build.py, as self_attn.hip).
#include "common.h"

namespace nabu {

constexpr int CM_TT = 32;                        // frames a workgroup owns (nabu_conv_module_tile_t)

struct CmArgs {
  const float *u, *w, *bw, *gamma, *beta, *mean, *rstd, *dy, *dz;
  float *y, *mean_out, *rstd_out, *du, *dz_out, *part_ln, *part_dw;
  const int32_t *len;
  int B, T, D, K, ld;
  float eps;
};

__device__ __forceinline__ float cm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the K taps of channel c centred among KC registers
template <int KC>
__device__ __forceinline__ void cm_load_taps(const CmArgs &a, int c, float (&w)[KC]) {
  const int off = (KC - a.K) / 2;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    const int k = j - off;
    w[j] = (k >= 0 && k < a.K) ? a.w[(size_t)k * a.D + c] : 0.f;
  }
}

// Phase 1 of the forward and of the first backward kernel: z of frames t0 .. t0 + rows - 1 of utterance b into zs[rows][D]
template <int KC>
__device__ __forceinline__ void cm_conv_tile(const CmArgs &a, int b, int t0, int len, int rows, float *zs) {
  constexpr int HC = (KC - 1) / 2, RPB = 31 / KC, STEPS = KC * RPB, LB = STEPS;
  const int nsteps = rows + KC - 1, D = a.D;
  for (int c = threadIdx.x; c < D; c += 256) {
    float w[KC], win[KC], la[LB], lb[LB];
    cm_load_taps<KC>(a, c, w);
#pragma unroll
    for (int j = 0; j < KC; ++j) win[j] = 0.f;
    const float bias = a.bw[c];
    const float *ub = a.u + (size_t)b * a.T * a.ld + c;
    for (int s0 = 0; s0 < nsteps; s0 += STEPS) {
#pragma unroll
      for (int j = 0; j < STEPS; ++j) {
        if (j % LB == 0) {
#pragma unroll
          for (int i = 0; i < LB; ++i) {
            const int tc = min(max(t0 - HC + s0 + j + i, 0), len - 1);       // a frame that exists; selected away below
            la[i] = ub[(size_t)tc * a.ld];
            lb[i] = ub[(size_t)tc * a.ld + D];
          }
        }
        const int s = s0 + j, t = t0 - HC + s;
        if (s < nsteps) {                                                    // (uniform)
          win[j % KC] = (t >= 0 && t < len) ? la[j % LB] * cm_sigmoid(lb[j % LB]) : 0.f;
          if (s >= KC - 1) {
            float z = bias;
#pragma unroll
            for (int k = 0; k < KC; ++k) z = fmaf(w[k], win[(j + 1 + k) % KC], z);
            zs[(s - (KC - 1)) * D + c] = z;
          }
        }
      }
    }
  }
}

template <int KC>
__global__ __launch_bounds__(256) void cm_fwd_kernel(CmArgs a) {
  extern __shared__ float zs[];                                              // [CM_TT][D]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * CM_TT, D = a.D;
  const int len = min(max(a.len[b], 0), a.T);
  const int rows = min(CM_TT, len - t0), trows = min(CM_TT, a.T - t0);       // frames that exist, frames of the buffer
  const size_t row0 = (size_t)b * a.T + t0;
  for (int i = max(rows, 0) * D + tid; i < trows * D; i += 256) a.y[row0 * D + i] = 0.f;
  for (int f = max(rows, 0) + tid; f < trows; f += 256) a.mean_out[row0 + f] = a.rstd_out[row0 + f] = 0.f;
  if (rows <= 0) return;                                                     // a tile of padding frames: zeros, nothing else
  cm_conv_tile<KC>(a, b, t0, len, rows, zs);
  __syncthreads();
  const float inv_d = 1.0f / (float)D;
  for (int f = wv; f < rows; f += 4) {
    const float *z = zs + f * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += z[c];
    const float mu = wave_sum(s) * inv_d;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) q = fmaf(z[c] - mu, z[c] - mu, q);
    const float rs = 1.0f / sqrtf(wave_sum(q) * inv_d + a.eps);
    for (int c = lane; c < D; c += 64) {
      const float n = fmaf(a.gamma[c], (z[c] - mu) * rs, a.beta[c]);
      a.y[(row0 + f) * D + c] = n * cm_sigmoid(n);
    }
    if (lane == 0) {
      a.mean_out[row0 + f] = mu;
      a.rstd_out[row0 + f] = rs;
    }
  }
}

// part_ln row of a workgroup: [dgamma | dbeta | dbw], 3 D wide
template <int KC>
__global__ __launch_bounds__(256) void cm_bwd_norm_kernel(CmArgs a) {
  extern __shared__ float zs[];                                              // [CM_TT][D], then [4 waves][3][D]
  constexpr int NI = 16;                                                     // D / 64 <= 16 channels per lane
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * CM_TT, D = a.D, nd = D / 64;
  const int len = min(max(a.len[b], 0), a.T);
  const int rows = min(CM_TT, len - t0), trows = min(CM_TT, a.T - t0);
  const size_t row0 = (size_t)b * a.T + t0;
  float *part = a.part_ln + ((size_t)b * gridDim.x + blockIdx.x) * 3 * D;
  for (int i = max(rows, 0) * D + tid; i < trows * D; i += 256) a.dz_out[row0 * D + i] = 0.f;
  if (rows <= 0) {
    for (int i = tid; i < 3 * D; i += 256) part[i] = 0.f;
    return;
  }
  cm_conv_tile<KC>(a, b, t0, len, rows, zs);
  __syncthreads();
  const float inv_d = 1.0f / (float)D;
  float ag[NI], ab[NI], az[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) ag[i] = ab[i] = az[i] = 0.f;
  for (int f = wv; f < rows; f += 4) {
    const float mu = a.mean[row0 + f], rs = a.rstd[row0 + f];
    const float *z = zs + f * D, *dy = a.dy + (row0 + f) * D;
    float dnh[NI], nh[NI], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < nd) {                                                          // (uniform)
        const int c = lane + 64 * i;
        const float g = a.gamma[c], zh = (z[c] - mu) * rs, n = fmaf(g, zh, a.beta[c]), sg = cm_sigmoid(n);
        const float dn = dy[c] * (sg * fmaf(n, 1.0f - sg, 1.0f));            // swish'(n) = s (1 + n (1 - s))
        ag[i] = fmaf(dn, zh, ag[i]);
        ab[i] += dn;
        dnh[i] = dn * g;
        nh[i] = zh;
        s1 += dnh[i];
        s2 = fmaf(dnh[i], zh, s2);
      }
    }
    s1 = wave_sum(s1) * inv_d;
    s2 = wave_sum(s2) * inv_d;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i < nd) {
        const float dz = rs * (dnh[i] - s1 - nh[i] * s2);
        a.dz_out[(row0 + f) * D + lane + 64 * i] = dz;
        az[i] += dz;
      }
    }
  }
  __syncthreads();                                                           // every wave is done with z
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (i < nd) {
      const int c = lane + 64 * i;
      zs[(wv * 3 + 0) * D + c] = ag[i];
      zs[(wv * 3 + 1) * D + c] = ab[i];
      zs[(wv * 3 + 2) * D + c] = az[i];
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * D; i += 256)                                     // i = q D + c; the four waves in order
    part[i] = ((zs[i] + zs[3 * D + i]) + zs[6 * D + i]) + zs[9 * D + i];
}

// part_dw row of a workgroup: [K][D]; grid (time tiles, chunks of 256 channels, B)
template <int KC>
__global__ __launch_bounds__(256) void cm_bwd_conv_kernel(CmArgs a) {
  constexpr int HC = (KC - 1) / 2, RPB = 31 / KC, STEPS = KC * RPB, LB = KC == 31 ? 8 : KC == 15 ? 15 : 14;
  const int b = blockIdx.z, t0 = blockIdx.x * CM_TT, D = a.D, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= D) return;
  const int len = min(max(a.len[b], 0), a.T);
  const int rows = min(CM_TT, len - t0), trows = min(CM_TT, a.T - t0);
  const int off = (KC - a.K) / 2;
  float *part = a.part_dw + ((size_t)b * gridDim.x + blockIdx.x) * a.K * D + c;
  float *du = a.du + ((size_t)b * a.T + t0) * a.ld + c;
  for (int f = max(rows, 0); f < trows; ++f) du[(size_t)f * a.ld] = du[(size_t)f * a.ld + D] = 0.f;
  if (rows <= 0) {
    for (int k = 0; k < a.K; ++k) part[(size_t)k * D] = 0.f;
    return;
  }
  float w[KC], zwin[KC], gwin[KC], acc[KC], la[LB], lb[LB], lz[LB];
  cm_load_taps<KC>(a, c, w);
#pragma unroll
  for (int j = 0; j < KC; ++j) zwin[j] = gwin[j] = acc[j] = 0.f;
  const float *ub = a.u + (size_t)b * a.T * a.ld + c, *dzb = a.dz + (size_t)b * a.T * D + c;
  const int nsteps = rows + KC - 1;
  for (int s0 = 0; s0 < nsteps; s0 += STEPS) {
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
      if (j % LB == 0) {
#pragma unroll
        for (int i = 0; i < LB; ++i) {
          const int tc = min(max(t0 - HC + s0 + j + i, 0), len - 1);
          la[i] = ub[(size_t)tc * a.ld];
          lb[i] = ub[(size_t)tc * a.ld + D];
          lz[i] = dzb[(size_t)tc * D];
        }
      }
      const int s = s0 + j, t = t0 - HC + s;
      if (s < nsteps) {                                                      // (uniform)
        const bool valid = t >= 0 && t < len;
        gwin[j % KC] = valid ? la[j % LB] * cm_sigmoid(lb[j % LB]) : 0.f;
        zwin[j % KC] = valid ? lz[j % LB] : 0.f;
        if (s >= KC - 1) {                                                   // output frame t - HC: the windows' centre
          const int f = s - (KC - 1);
          const float dzc = zwin[(j + 1 + HC) % KC], gc = gwin[(j + 1 + HC) % KC];
          float dg = 0.f;
#pragma unroll
          for (int k = 0; k < KC; ++k) {
            dg = fmaf(w[k], zwin[(j + 1 + KC - 1 - k) % KC], dg);            // dz[t_out - k + HC]
            acc[k] = fmaf(dzc, gwin[(j + 1 + k) % KC], acc[k]);              // g[t_out + k - HC]
          }
          const float sg = cm_sigmoid(ub[(size_t)(t0 + f) * a.ld + D]);
          du[(size_t)f * a.ld] = dg * sg;
          du[(size_t)f * a.ld + D] = dg * (gc * (1.0f - sg));                // a sigmoid'(b) = g (1 - s)
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KC; ++j)
    if (j >= off && j < off + a.K) part[(size_t)(j - off) * D] = acc[j];
}

static int cm_check(const char *what, int B, int T, int D, int K, const float *u, int ld) {
  NABU_CHECK_ARG(B >= 0 && T >= 0, "%s: negative batch or time dimension", what);
  NABU_CHECK_ARG(D >= 64 && D % 64 == 0 && D <= 1024, "%s: D = %d, must be a multiple of 64 in 64..1024", what, D);
  NABU_CHECK_ARG(K >= 3 && K <= 31 && K % 2 == 1, "%s: K = %d, must be odd in 3..31", what, K);
  NABU_CHECK_ARG(ld >= 2 * D, "%s: ld = %d < 2 D = %d", what, ld, 2 * D);
  NABU_CHECK_ARG(ld % 4 == 0, "%s: ld = %d is not a multiple of 4", what, ld);
  NABU_CHECK_ARG(B <= 65535, "%s: B = %d > 65535", what, B);
  NABU_CHECK_ARG((reinterpret_cast<uintptr_t>(u) & 15) == 0, "%s: u must be 16-byte aligned", what);
  return 0;
}

// the tap class of K
#define CM_DISPATCH(K, CALL)             \
  do {                                   \
    if ((K) <= 7) { CALL(7); }           \
    else if ((K) <= 15) { CALL(15); }    \
    else { CALL(31); }                   \
  } while (0)

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_conv_module_tile_t(void) { return CM_TT; }
extern "C" int nabu_conv_module_parts(int B, int T) { return B * ((T + CM_TT - 1) / CM_TT); }

extern "C" int nabu_conv_module_fwd(int B, int T, int D, int K, const float *u, int ld, const int32_t *len, const float *w,
                                    const float *bw, const float *gamma, const float *beta, float eps, float *y,
                                    float *mean, float *rstd, nabu_stream_t stream) {
  NABU_CHECK_ARG(u && len && w && bw && gamma && beta && y && mean && rstd, "conv_module_fwd: null pointer");
  NABU_TRY(cm_check("conv_module_fwd", B, T, D, K, u, ld));
  if (B == 0 || T == 0) return 0;
  CmArgs a = {};
  a.u = u; a.len = len; a.w = w; a.bw = bw; a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.y = y; a.mean_out = mean; a.rstd_out = rstd;
  a.B = B; a.T = T; a.D = D; a.K = K; a.ld = ld;
  const dim3 grid((T + CM_TT - 1) / CM_TT, B);
  const size_t lds = (size_t)CM_TT * D * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int e = 0;
#define CM_FWD(KC) e = launch_lds(cm_fwd_kernel<KC>, grid, dim3(256), lds, s, a)
  CM_DISPATCH(K, CM_FWD);
#undef CM_FWD
  return e;
}

extern "C" int nabu_conv_module_bwd(int B, int T, int D, int K, const float *u, int ld, const int32_t *len, const float *w,
                                    const float *bw, const float *gamma, const float *beta, const float *mean,
                                    const float *rstd, const float *dy, float *du, float *dz, float *part_ln,
                                    float *part_dw, nabu_stream_t stream) {
  NABU_CHECK_ARG(u && len && w && bw && gamma && beta && mean && rstd && dy && du && dz && part_ln && part_dw,
                 "conv_module_bwd: null pointer");
  NABU_TRY(cm_check("conv_module_bwd", B, T, D, K, u, ld));
  if (B == 0 || T == 0) return 0;
  CmArgs a = {};
  a.u = u; a.len = len; a.w = w; a.bw = bw; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd; a.dy = dy;
  a.du = du; a.dz_out = dz; a.dz = dz; a.part_ln = part_ln; a.part_dw = part_dw;
  a.B = B; a.T = T; a.D = D; a.K = K; a.ld = ld;
  const int tiles = (T + CM_TT - 1) / CM_TT;
  const size_t lds = (size_t)CM_TT * D * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define CM_BWD(KC)                                                                                  \
  NABU_TRY(launch_lds(cm_bwd_norm_kernel<KC>, dim3(tiles, B), dim3(256), lds, s, a));               \
  hipLaunchKernelGGL(cm_bwd_conv_kernel<KC>, dim3(tiles, (D + 255) / 256, B), dim3(256), 0, s, a)
  CM_DISPATCH(K, CM_BWD);
#undef CM_BWD
  NABU_LAUNCH_CHECK();
  return 0;
}
