// speller_attn_dev.h — device helpers shared by the attention kernels of speller.hip (one memory) and speller_multi.hip
// (M memories in one launch): the hand-off between the frame slices of an utterance inside a launch, and the location
// features.
#pragma once
#include "common.h"

namespace nabu {

constexpr int AT = 512;   // threads per attention workgroup (8 wave64)

// store / load of data handed from one workgroup to another inside a launch: write-through store, L1-bypassing
// load (MI355X_MICROARCH.md "sc1 stores AND sc1 loads"); plain (x = false) when the hand-off is a kernel boundary
__device__ __forceinline__ void xst(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xst(float *p, float v, bool x) {
  if (x) xst(p, v);
  else   *p = v;
}
__device__ __forceinline__ float xld(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// every wave has drained its stores; returns true in the workgroup that arrives last of n (the counter is left zero,
// ready for reuse)
__device__ __forceinline__ bool last_arriver(unsigned *ticket, unsigned n, int *flag) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = old == n - 1;
    if (old == n - 1) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return *flag != 0;
}

// the conv kernel [K*F] of location-aware attention (kind 1) is staged at the start of the dynamic LDS: its floats, a
// 16-byte multiple
__host__ __device__ __forceinline__ int ck_floats(int kind, int K, int F) { return kind == 1 ? (K * F + 3) & ~3 : 0; }
// cf[t,f] = sum_d a[t + d - pb] ck[d,f], 'same' padding, pb = (K-1)/2 (tf.layers.conv1d); frames [lo,hi)
__device__ __forceinline__ void conv_features(int K, int F, int Te, const float *al_prev, float *cf, int lo, int hi,
                                              const float *ck_s) {
  const int pb = (K - 1) / 2;
  for (int i = lo * F + threadIdx.x; i < hi * F; i += AT) {
    const int t = i / F, f = i % F;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;     // independent chains: the loop is LDS-latency bound
    const int d0 = max(0, pb - t), d1 = min(K, Te + pb - t);
    const float *a = al_prev + t - pb, *c = ck_s + f;
    int d = d0;
    for (; d + 3 < d1; d += 4) {
      s0 = fmaf(a[d], c[d * F], s0);
      s1 = fmaf(a[d + 1], c[(d + 1) * F], s1);
      s2 = fmaf(a[d + 2], c[(d + 2) * F], s2);
      s3 = fmaf(a[d + 3], c[(d + 3) * F], s3);
    }
    for (; d < d1; ++d) s0 = fmaf(a[d], c[d * F], s0);
    cf[i] = (s0 + s1) + (s2 + s3);
  }
}

}  // namespace nabu
