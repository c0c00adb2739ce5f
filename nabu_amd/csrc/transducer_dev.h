// transducer_dev.h — what the transducer's lattice kernels share: the loss (transducer.hip) and the forced alignment
// (transducer_align.hip) work on the SAME per-node terms, so the expression that makes them is written once, here.
#pragma once
#include "common.h"

namespace nabu {

constexpr float TR_NEG = -1e30f;    // unreachable (CTC_NEG of ctc.hip): -1e30 + x is -1e30 again, never inf - inf
constexpr int TR_NT = 256;
constexpr int TR_AHEAD = 8;         // diagonals per group of loads of the wave routes

__device__ __forceinline__ int tr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float tr_up(float v, float fill) {     // lane i <- lane i-1 (lane 0 <- fill)
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x138, 0xf, 0xf, false));
}

// The terms of one lattice node from its two logit rows: the node's own maximum m and log-sum l of h = fr + gr (one
// float32 addition per class), lb = log p(blank), ly = log p(lab) (unreachable for lab < 0); maximum and log-sum kept
// apart, as in ctc_kernel
__device__ __forceinline__ void tr_node_terms(const float *fr, const float *gr, int C, int lab, float *m_out, float *l_out,
                                              float *lb, float *ly) {
  const int blank = C - 1;
  float m = fr[0] + gr[0];
  for (int k = 1; k < C; ++k) m = fmaxf(m, fr[k] + gr[k]);
  float z = 0.f;
  for (int k = 0; k < C; ++k) z += expf((fr[k] + gr[k]) - m);
  const float l = logf(z);
  *m_out = m;
  *l_out = l;
  *lb = ((fr[blank] + gr[blank]) - m) - l;
  *ly = lab >= 0 ? ((fr[lab] + gr[lab]) - m) - l : TR_NEG;
}

// the verdict on utterance b, the same in every thread of the workgroup (one barrier)
__device__ __forceinline__ bool tr_lengths_labels_bad(int T, int U1, int C, const int32_t *enc_len, const int32_t *labels,
                                                      int ldl, const int32_t *label_len, int b, int tid, int nt) {
  const int Tb = enc_len[b], Ub = label_len[b];
  int bad = (Tb <= 0 || Tb > T || Ub < 0 || Ub > U1 - 1) ? 1 : 0;
  if (!bad)
    for (int u = tid; u < Ub; u += nt) {
      const int l = labels[(size_t)b * ldl + u];
      if (l < 0 || l >= C - 1) bad = 1;
    }
  return __syncthreads_or(bad) != 0;
}

// ctc_align's rule: atomicCAS(status, 0, b + 1), repeated while a LATER utterance holds the word
__device__ __forceinline__ void tr_status_first(int32_t *status, int b) {
  const int want = b + 1;
  int old = atomicCAS(status, 0, want);
  while (old != 0 && old > want) {
    const int seen = atomicCAS(status, old, want);
    if (seen == old) break;
    old = seen;
  }
}

}  // namespace nabu
