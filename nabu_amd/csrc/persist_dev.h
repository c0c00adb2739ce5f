// persist_dev.h — device primitives shared by ALL persistent kernels (the recurrences of lstm_persist*.hip through
// lstm_persist_dev.h, the decoder of speller_persist.hip): the sentinel of the exchange rings, the exchange stores and
// load, the gate functions.
#pragma once
#include "common.h"

namespace nabu {

constexpr unsigned SENT = 0xFFFFFFFFu;   // a ring word nobody has published yet (the rings start as 0xFF bytes)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool has_sentinel(const u32x4 v) {
  return v.x == SENT || v.y == SENT || v.z == SENT || v.w == SENT;
}
__device__ __forceinline__ bool all_sentinel(const u32x4 v) {
  return v.x == SENT && v.y == SENT && v.z == SENT && v.w == SENT;
}

// Gate functions.  v_rcp_f32 is good to one unit in the last place but not centred (mean -0.06 .. -0.08 ulp on [1, 2),
// tools/experiments/ub/rcp_bias.hip), and 2 r - 1 turns that into a RELATIVE bias of tanh that grows as tanh shrinks: one
// cell update came out 3e-8 low in h on average (tools/experiments/ub/cell_bias.hip; the step kernels' true divisions:
// 4e-9) — invisible in any single value, but a sum over 32 000 frames (a bias gradient) or a thousand dependent steps
// collects it: at T = 1000 the persistent kernels' gradients stood at 1.4-5 x the step kernels' error against float64.
// So: one Newton step behind the reciprocal (two fused multiply-adds: centred again, mean as the division's), and tanh
// as (1 - e) / (1 + e), whose numerator cancels nothing behind the reciprocal (half the rms error of 2 r - 1 besides);
// the clamp keeps e = exp(-2x) finite (|tanh| = 1 to the last bit beyond |x| = 9 already).
// The Newton step cannot take d = inf (r = 0, and -inf * 0 + 1 is NaN), and exp(-x) is inf below x = -88.73: a gate
// pre-activation that low (a large negative bias, a saturating weight column) turned the gate, the rest of the sequence
// and every gradient into NaN where the function is 0 (tests/test_hip_recurrence_range.py).  So x < -88.7 (exp still
// finite there: 3.3e38, sigmoid 3.0e-39) takes 0 — the input the select is for is a gate pre-activation below -88.7,
// -inf included.  A compare that fails for NaN, so a NaN argument stays NaN, and every x >= -88.7 gives the bits it always
// gave.  The RESULT is selected, not the argument clamped: the compare then runs beside the exponential and one
// v_cndmask_b32 per gate is all the chain sees; compare + select in front of v_exp_f32 cost 0.2 ms of cfg2's 12.0 ms
// step (LABNOTES section 23).
__device__ __forceinline__ float rcp_newton(float d) {
  const float r = __builtin_amdgcn_rcpf(d);
  return fmaf(fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ float fast_sigmoid(float x) {
  const float s = rcp_newton(1.0f + __expf(-x));
  return x < -88.7f ? 0.0f : s;
}
__device__ __forceinline__ float fast_tanh(float x) {
  const float e = __expf(-2.0f * __builtin_amdgcn_fmed3f(x, -30.0f, 30.0f));
  return (1.0f - e) * rcp_newton(1.0f + e);
}

// stores of the exchange, 16 and 4 bytes: plain when the whole unit shares one L2, else write-through; its load
// bypasses the L1
__device__ __forceinline__ void xstore(const u32x4 v, __amdgpu_buffer_rsrc_t rs, unsigned off, bool coloc) {
  if (coloc) __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 0);
  else       __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 16);
}
__device__ __forceinline__ void xstore1(unsigned v, __amdgpu_buffer_rsrc_t rs, unsigned off, bool coloc) {
  if (coloc) __builtin_amdgcn_raw_buffer_store_b32(v, rs, off, 0, 0);
  else       __builtin_amdgcn_raw_buffer_store_b32(v, rs, off, 0, 16);
}
__device__ __forceinline__ u32x4 xload(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
}

}  // namespace nabu
