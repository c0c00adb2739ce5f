// attn_drop.h — the dropout mask of the attention probabilities, shared by self_attn.hip and self_attn_bf16.hip
// (nabu_self_attn_drop_* / nabu_self_attn_bf16_drop_*, include/nabu_hip.h).
//
// THE MASK is a function of (seed, offset, b, h, q, k) only — not of T, of a tile size, of the kernel that asks or of
// the precision: element (b, h, q, k) is word k & 3 of the Philox4x32-10 block with counter (g_lo, g_hi, offset_lo,
// offset_hi), key (seed_lo, seed_hi) and g = ((b H + h) << 38) | (q << 18) | (k >> 2); it is kept when u01(word) < keep
// (compared in float32) and then scaled by fl(1 / keep): the rule of dropout_scale4 (common.h).  q < 2^20 is what the
// entry points' refusal of T > 2^20 buys; b H + h < 2^21 (B <= 65535, H <= 32).
//
// The kernels never hold scale factors: a 32 x 32 score tile's mask is 16 KEEP BITS per lane, bit r for accumulator
// register r, made before the tile's S product is issued (integer VALU and v_mad_u64_u32, independent of the matrix
// pipe) and spent as one select and one multiply per probability.
//   * lane = query (forward, dQ): registers 4 g .. 4 g + 3 of half-wave lk are keys kbase + 8 g + 4 lk + 0..3 of the
//     lane's query — four consecutive keys aligned to four, ONE block: four blocks per lane and 32 keys.
//   * lane = key (dK/dV): registers 4 g .. 4 g + 3 are queries qbase + 8 g + 4 lk + 0..3 of the lane's key, four
//     DIFFERENT blocks, and the four lanes of a quad (keys 4 j .. 4 j + 3, one half-wave) need the same sixteen.  Lane c
//     of the quad computes the four blocks of register group g = c (all four words of each: 16 bits, bit 4 i + j = query
//     i of the group, key j of the quad); four DPP quad broadcasts hand every lane the four words, from which it picks
//     its own key's column.  Four blocks per lane and tile, as where a lane is a query; no LDS, no barrier.
#pragma once
#include <math.h>

#include "common.h"

namespace nabu {

constexpr int ATTN_DROP_MAX_T = 1 << 20;         // the counter holds 20 bits of the query index and 18 of k >> 2

struct AttnDrop {                                // rides at the end of the kernels' argument structs
  float keep, inv;                               // keep probability; fl(1 / keep), divided on the host
  unsigned seed_lo, seed_hi, off_lo, off_hi;
};

// the refusals the dropout entry points add to the plain ones', and the mask's arguments
inline int attn_drop_args(const char *what, int T, float keep, unsigned long long seed, unsigned long long offset,
                          AttnDrop *d) {
  NABU_CHECK_ARG(T <= ATTN_DROP_MAX_T, "%s: T = %d > 2^20 = %d (the mask's counter holds 20 bits of the frame index)", what,
                 T, ATTN_DROP_MAX_T);
  NABU_CHECK_ARG(isfinite(keep) && keep > 0.f && keep <= 1.f, "%s: keep = %g, must be a finite number in (0, 1]", what,
                 (double)keep);
  d->keep = keep; d->inv = 1.0f / keep;
  d->seed_lo = (unsigned)seed; d->seed_hi = (unsigned)(seed >> 32);
  d->off_lo = (unsigned)offset; d->off_hi = (unsigned)(offset >> 32);
  return 0;
}

// keep bits of keys 4 kg .. 4 kg + 3 of query q of head bh = b H + h: bit j is set when key 4 kg + j is kept
__device__ __forceinline__ unsigned attn_keep4(const AttnDrop &d, unsigned bh, unsigned q, unsigned kg) {
  const uint4 r = philox4x32_10(make_uint4((q << 18) | kg, (bh << 6) | (q >> 14), d.off_lo, d.off_hi),
                                make_uint2(d.seed_lo, d.seed_hi));
  return (u01(r.x) < d.keep ? 1u : 0u) | (u01(r.y) < d.keep ? 2u : 0u) | (u01(r.z) < d.keep ? 4u : 0u) |
         (u01(r.w) < d.keep ? 8u : 0u);
}

// lane = query q: bit r is key kbase + acc_row(r, lk) (kbase a multiple of 32)
__device__ __forceinline__ unsigned attn_keep16_query(const AttnDrop &d, unsigned bh, int q, int kbase, int lk) {
  unsigned m = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) m |= attn_keep4(d, bh, q, (kbase >> 2) + 2 * g + lk) << (4 * g);
  return m;
}

template <int G>
__device__ __forceinline__ unsigned quad_broadcast(unsigned x) {       // lane G of every quad, to its four lanes
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, G * 0x55, 0xf, 0xf, true);
}

// bits 0, 4, 8, 12 of x (and no others set) -> bits 0..3
__device__ __forceinline__ unsigned gather4(unsigned x) { return (x | (x >> 3) | (x >> 6) | (x >> 9)) & 15u; }

// lane = key ki: bit r is query qbase + acc_row(r, lk) (qbase a multiple of 32).  Every lane of the wave must be here.
__device__ __forceinline__ unsigned attn_keep16_key(const AttnDrop &d, unsigned bh, int qbase, int ki, int lk, int lane) {
  const int c = lane & 3;
  unsigned mine = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) mine |= attn_keep4(d, bh, qbase + 8 * c + 4 * lk + i, ki >> 2) << (4 * i);
  return gather4((quad_broadcast<0>(mine) >> c) & 0x1111u) | gather4((quad_broadcast<1>(mine) >> c) & 0x1111u) << 4 |
         gather4((quad_broadcast<2>(mine) >> c) & 0x1111u) << 8 | gather4((quad_broadcast<3>(mine) >> c) & 0x1111u) << 12;
}

// the scale factor of register r: fl(1 / keep) or +0.0
__device__ __forceinline__ float attn_drop_scale(const AttnDrop &d, unsigned bits, int r) {
  return (bits >> r) & 1u ? d.inv : 0.f;
}

}  // namespace nabu
