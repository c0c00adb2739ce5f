// specaug.hip — SpecAugment on the encoder's input features: a linear time warp about one random anchor frame, then
// time masks and frequency masks that write zeros (include/nabu_hip.h, nabu_spec_augment_f32; the rules: DESIGN.md).
//
// One launch.  Utterance b is a slab of T * D contiguous floats; blockIdx.y = b, blockIdx.x = a run of SA_GROUPS groups
// of 4 consecutive output floats.  A group is the 16 bytes at an ALIGNED address of y: rows of D = 123 floats start at
// any of the four float offsets, so the groups are cut by the address of y, not by the row (the slab's first and last
// group may be partial: scalar stores).  The source of an output float is found per element — the same flat index
// (masks only), or rows i and i + 1 of the warped utterance: one aligned 16-byte load of x serves the elements of a
// group that stay in place, 4-byte loads the elements of warped rows.
//
// Every workgroup derives its utterance's parameters itself: thread k < 1 + mT + mF draws Philox words (b, k, offset)
// and turns them into (c, c'), a time mask or a frequency mask in integer arithmetic; then one thread per row of the
// workgroup's run works out the row's source (one 64-bit division per row and workgroup, not per element) into LDS.
#include "common.h"

namespace nabu {

constexpr int SA_MAX_MASKS = 8;
constexpr int SA_GROUPS = 512;               // groups of 4 floats per workgroup (2 per thread)
constexpr int SA_ROWS = 4 * SA_GROUPS + 2;   // rows such a run can touch at D = 1, plus the partial ones at its ends

struct SpecAugArgs {
  int T, D, Dblk, W, mT, Tw, mF, Fw;
  float ratio;
  unsigned long long seed, offset;
};

// uniform integer in [0, m) from one Philox word: the word's upper 24 bits times m, in 64 bits
__device__ __forceinline__ int below(unsigned w, int m) {
  return (int)(((unsigned long long)(w >> 8) * (unsigned long long)(unsigned)m) >> 24);
}

__global__ __launch_bounds__(256) void spec_augment_kernel(SpecAugArgs a, const float *__restrict__ x,
                                                           const int32_t *__restrict__ len, float *__restrict__ y,
                                                           int32_t *__restrict__ params) {
  __shared__ int prm[2 + 4 * SA_MAX_MASKS];   // c, c', (t0, t) x mT, (f0, f) x mF
  __shared__ int row_src[SA_ROWS];            // source row of an output row; -1: the row is zero
  __shared__ float row_frac[SA_ROWS];         // weight of source row + 1 (0: the source row alone)
  const int b = blockIdx.y, tid = threadIdx.x, D = a.D;
  const unsigned TD = (unsigned)a.T * (unsigned)D;
  const float *xs = x + (size_t)b * TD;
  float *ys = y + (size_t)b * TD;
  const unsigned s = (unsigned)(reinterpret_cast<uintptr_t>(ys) >> 2) & 3u;   // floats of the first group before ys
  const unsigned ngroups = (TD + s + 3) / 4;
  const unsigned q0 = blockIdx.x * SA_GROUPS;
  if (q0 >= ngroups) return;
  const unsigned q1 = min(q0 + SA_GROUPS, ngroups);
  const int n = min(max(len[b], 0), a.T);
  const int np = 2 + 2 * a.mT + 2 * a.mF;

  if (tid < 1 + a.mT + a.mF) {
    const uint4 r = philox4x32_10(make_uint4((unsigned)b, (unsigned)tid, (unsigned)a.offset, (unsigned)(a.offset >> 32)),
                                  make_uint2((unsigned)a.seed, (unsigned)(a.seed >> 32)));
    if (tid == 0) {
      int c = 0, cp = 0;
      if (a.W > 0 && n >= 2 * a.W + 3) {
        c = a.W + 1 + below(r.x, n - 2 * a.W - 2);
        cp = c - a.W + below(r.y, 2 * a.W + 1);
      }
      prm[0] = c;
      prm[1] = cp;
    } else if (tid <= a.mT) {
      const int cap = min(a.Tw, (int)(a.ratio * (float)n));
      const int t = below(r.x, cap + 1);
      prm[2 * tid] = below(r.y, n - t + 1);
      prm[2 * tid + 1] = t;
    } else {
      const int f = below(r.x, min(a.Fw, a.Dblk) + 1);
      prm[2 * tid] = below(r.y, a.Dblk - f + 1);
      prm[2 * tid + 1] = f;
    }
  }
  __syncthreads();
  if (params && blockIdx.x == 0 && tid < np) params[(size_t)b * np + tid] = prm[tid];

  // rows of this run's first and last element
  const unsigned e_first = 4 * q0 > s ? 4 * q0 - s : 0u;
  const unsigned e_last = min(4 * q1 - s, TD) - 1;
  const int r_first = (int)(e_first / (unsigned)D), r_last = (int)(e_last / (unsigned)D);
  const int c = prm[0], cp = prm[1];
  for (int t = r_first + tid; t <= r_last; t += 256) {
    int src = t;
    float fr = 0.f;
    if (t < n) {
      bool zero = false;
      for (int j = 0; j < a.mT; ++j) zero |= (unsigned)(t - prm[2 + 2 * j]) < (unsigned)prm[3 + 2 * j];
      if (zero) {
        src = -1;
      } else if (c > 0) {
        // frames 0, c', n - 1 read frames 0, c, n - 1; linear in between (1 <= c' <= n - 2: both denominators >= 1)
        unsigned long long num, den;
        if (t < cp) {
          num = (unsigned long long)t * c;
          den = cp;
        } else {
          den = n - 1 - cp;
          num = (unsigned long long)c * den + (unsigned long long)(t - cp) * (n - 1 - c);
        }
        const unsigned long long i = num / den, rem = num - i * den;
        src = (int)i;
        fr = (float)(unsigned)rem / (float)(unsigned)den;       // rem > 0 only for i < n - 1
      }
    }
    row_src[t - r_first] = src;
    row_frac[t - r_first] = fr;
  }
  __syncthreads();

  const int mF = a.mF, Dblk = a.Dblk;
  const int *fm = prm + 2 + 2 * a.mT;
  for (unsigned q = q0 + tid; q < q1; q += 256) {
    const long long e0 = 4ll * q - s;                            // slab index of the group's first float (< 0: before ys)
    const int jlo = e0 < 0 ? (int)-e0 : 0;
    const int jhi = (long long)TD - e0 < 4 ? (int)((long long)TD - e0) : 4;
    const unsigned e = (unsigned)(e0 + jlo);
    int t = (int)(e / (unsigned)D);
    int d = (int)(e - (unsigned)t * (unsigned)D);
    int dk = d % Dblk;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const bool whole = jlo == 0 && jhi == 4;
    // 16 aligned bytes of x under a whole group: one load serves every element whose source is its own place (a row
    // that is not warped) — with masks only, all of them, also where the group runs across the end of a row
    const bool have = whole && (reinterpret_cast<uintptr_t>(xs + e) & 15) == 0;
    float xv[4] = {0.f, 0.f, 0.f, 0.f};
    if (have) {
      const float4 q4 = *reinterpret_cast<const float4 *>(xs + e);
      xv[0] = q4.x; xv[1] = q4.y; xv[2] = q4.z; xv[3] = q4.w;
    }
    int src = row_src[t - r_first];
    float fr = row_frac[t - r_first];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < jlo || j >= jhi) continue;
      bool zero = src < 0;
      if (!zero && t < n)
        for (int k = 0; k < mF; ++k) zero |= (unsigned)(dk - fm[2 * k]) < (unsigned)fm[2 * k + 1];
      if (!zero) {
        if (have && src == t && fr == 0.f) {
          v[j] = xv[j];
        } else {
          const float *p = xs + (size_t)src * D + d;
          float val = p[0];
          if (fr != 0.f) val = fmaf(fr, p[D] - val, val);
          v[j] = val;
        }
      }
      if (++dk == Dblk) dk = 0;
      if (++d == D) {
        d = 0;
        ++t;
        if (j + 1 < jhi) {        // (the run's row table ends at its last element's row)
          src = row_src[t - r_first];
          fr = row_frac[t - r_first];
        }
      }
    }
    if (whole) {
      *reinterpret_cast<float4 *>(ys + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j >= jlo && j < jhi) ys[e0 + j] = v[j];
    }
  }
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_spec_augment_f32(const nabu_specaug_desc *desc, const float *x, const int32_t *len, float *y,
                                     int32_t *params, unsigned long long seed, unsigned long long offset,
                                     nabu_stream_t stream) {
  NABU_CHECK_ARG(desc && desc->size >= sizeof(nabu_specaug_desc), "spec_augment: null or short descriptor");
  const nabu_specaug_desc &d = *desc;
  NABU_CHECK_ARG(d.B >= 0 && d.T >= 0 && d.D >= 0, "spec_augment: negative shape B=%d T=%d D=%d", d.B, d.T, d.D);
  NABU_CHECK_ARG(d.time_warp >= 0 && d.time_warp < (1 << 24), "spec_augment: time_warp = %d", d.time_warp);
  NABU_CHECK_ARG(d.time_masks >= 0 && d.time_masks <= SA_MAX_MASKS, "spec_augment: time_masks = %d outside 0..%d",
                 d.time_masks, SA_MAX_MASKS);
  NABU_CHECK_ARG(d.freq_masks >= 0 && d.freq_masks <= SA_MAX_MASKS, "spec_augment: freq_masks = %d outside 0..%d",
                 d.freq_masks, SA_MAX_MASKS);
  NABU_CHECK_ARG(d.time_mask_width >= 0 && d.freq_mask_width >= 0, "spec_augment: negative mask width");
  NABU_CHECK_ARG(d.time_mask_ratio > 0.f && d.time_mask_ratio <= 1.f, "spec_augment: time_mask_ratio = %g outside (0, 1]",
                 (double)d.time_mask_ratio);
  NABU_CHECK_ARG(d.feature_blocks >= 1, "spec_augment: feature_blocks = %d", d.feature_blocks);
  if (d.B == 0 || d.T == 0 || d.D == 0) return 0;
  NABU_CHECK_ARG(d.D % d.feature_blocks == 0, "spec_augment: D = %d is not a multiple of feature_blocks = %d", d.D,
                 d.feature_blocks);
  NABU_CHECK_ARG(x && y && len, "spec_augment: null pointer");
  NABU_CHECK_ARG(((uintptr_t)x | (uintptr_t)y | (uintptr_t)len | (uintptr_t)params) % 4 == 0,
                 "spec_augment: a pointer is not 4-byte aligned");
  // n < 2^24: (float)n and the warp's remainders are exact in float32
  if (d.T >= (1 << 24)) return fail(NABU_EUNSUP, "spec_augment: T = %d >= 2^24", d.T);
  if ((unsigned long long)d.T * d.D > 0x7FFFFFF0ull)
    return fail(NABU_EUNSUP, "spec_augment: an utterance of T * D = %d * %d floats", d.T, d.D);
  if (d.B > 65535) return fail(NABU_EUNSUP, "spec_augment: B = %d > 65535", d.B);
  const size_t total = (size_t)d.B * d.T * d.D;
  NABU_CHECK_ARG(x + total <= y || y + total <= x, "spec_augment: x and y overlap (the call is out of place)");
  SpecAugArgs a = {d.T, d.D, d.D / d.feature_blocks, d.time_warp, d.time_masks, d.time_mask_width, d.freq_masks,
                   d.freq_mask_width, d.time_mask_ratio, seed, offset};
  const unsigned groups = (unsigned)(((unsigned long long)d.T * d.D + 6) / 4);    // at most, whatever y's alignment
  hipLaunchKernelGGL(spec_augment_kernel, dim3((groups + SA_GROUPS - 1) / SA_GROUPS, d.B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, x, len, y, params);
  NABU_LAUNCH_CHECK();
  return 0;
}
