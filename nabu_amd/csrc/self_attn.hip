// self_attn.hip — the self-attention encoder's one new operation: multi-head scaled dot-product attention of a padded
// batch over ALL pairs of frames of an utterance, forward and backward, fp32 on v_mfma_f32_32x32x2_f32.  The T x T score
// matrix exists only as accumulator registers, 32 x 32 at a time.
//
// Operands: qkv [B, T, 3 D] with row stride ld; Q, K, V are its three D-wide column blocks, head h is columns
// h dk .. (h+1) dk of each (dk 32 or 64: the template parameter DK).  len [B]: the length rule of include/nabu_hip.h.
//
// FORWARD (attn_fwd_kernel).  A workgroup of four waves owns ATTN_Q = 128 queries of one (b, h), a wave 32 of them; key
// and value tiles of ATTN_K = 32 rows stream through LDS, shared by the four waves and double-buffered (the next tile is
// fetched into registers under the current tile's matrix work, stored to the other buffer, ONE barrier per tile).
//   * The wave computes S^T = K Q^T, not S: M = keys, N = queries.  The B operand (Q^T) is the wave's own 32 queries, read
//     from memory once into DK / 2 registers; the A operand is the K tile in LDS.  In the 32 x 32 accumulator a lane then
//     holds ONE query's column: 16 keys in its registers, the other 16 in lane ^ 32.  The running maximum and sum of the
//     online softmax are in-lane reductions plus one exchange between the half-waves; no LDS round trip.
//   * The accumulator is fed straight back as the B operand of O^T = V^T P^T.  Register r of a lane holds key
//     kappa(r) + 4 (lane >> 5), kappa(r) = (r & 3) + 8 (r >> 2), and an MFMA step reduces over the two indices its
//     half-waves supply — so step r takes register r as B and V's rows kappa(r) (lanes 0..31) and kappa(r) + 4 (lanes
//     32..63) as A: the reduction index is permuted, V's rows are read from LDS in the same permuted order, and no
//     probability ever crosses a lane.  O^T's accumulator has the same lane = query layout, so the rescale by
//     exp(m_old - m_new) is in-lane too, and happens once per key tile.
//   * LDS rows have the ODD stride DK + 1: the S product reads a column of 32 keys (32 banks), the O product a row of 32
//     consecutive words.  Rows at or past len[b] are staged as zeros, whatever memory holds.
//   * The running maximum starts at -FLT_MAX and a masked key is left out by a select, never by an infinity: every tile
//     walked has a key below len[b], so the maximum is finite from the first tile on and exp(m_old - m_new) is 0 or finite.
// THE WINDOW (the WIN instantiations, nabu_self_attn_win_*; attn_win.h): query i sees keys lo(i) <= j < hi(i).  A lane
// computes its interval once in the prologue and tests (unsigned)(j - lo) < hi - lo where the plain kernels test j < len.
// A workgroup walks the key tiles from lo(its first query) / 32 to ceil(hi(its last query below len) / 32) - 1, tile
// boundaries still multiples of 32 counted from key 0 and the double buffer primed at the first walked tile; the dK/dV
// workgroup walks the query tiles from qlo(its first key) to qhi(its last key below len), and its predicate is the key's
// interval of queries (the lane's, with the query index running over the registers).  The walk depends on len[b], C and
// Lc only.  THE INVARIANT that replaces "every tile walked has a key below len": every query below len sees its own
// key, and the walk covers lo..hi of every query the workgroup owns, so every lane meets at least one key it sees —
// but not in every tile.  In a tile where a lane sees nothing, before its window or after it, the tile maximum stays
// -FLT_MAX, so m_new = m_old and the rescale is exp(0) = 1 exactly, also while m is still -FLT_MAX; all sixteen
// probabilities are selected to 0, so l and the accumulators keep their bits (l stays 0, m stays -FLT_MAX until the first
// seen key, where the rescale exp(-FLT_MAX - m_new) is 0 and multiplies zeros).  Nothing is ever left out by an infinity,
// and the backward kernels select P = exp(s - lse) to 0 outside the window whatever s is.  At the end l > 0 for every lane.
// BACKWARD, two kernels, each recomputing its score tiles from lse; no float atomics, no workspace, no reduce pass.
//   * attn_bwd_dq_kernel: the forward kernel's shape (queries owned, K and V tiles streamed).  S^T = K Q^T and
//     dP^T = V dO^T share the lane = query layout, so lse and delta = rowsum(dO . O) (computed in the prologue from the
//     registers that hold dO^T) are per-lane scalars; dS^T = P^T . (dP^T - delta) is fed back as the B operand of
//     dQ^T = K^T dS^T, K's rows read in the permuted order from the SAME LDS tile the S product read by columns.
//   * attn_bwd_dkv_kernel: the transpose.  A workgroup owns 128 KEYS, a wave 32 of them, K^T and V^T sit in registers as
//     B operands; Q and dO tiles of 32 queries stream through LDS (with lse and delta, which the staging threads compute
//     from dO and O as they load them).  S = Q K^T and dP = dO V^T have lane = key; P and dS are fed back as the B
//     operands of dV^T = dO^T P and dK^T = Q^T dS.
// Built with packed fp32 VALU instructions switched off (build.py, as conv2d.hip).
#include <float.h>

#include "attn_drop.h"
#include "attn_win.h"
#include "gemm_args.h"

namespace nabu {

constexpr int ATTN_Q = 128;                      // rows a workgroup owns: four waves x 32 (nabu_self_attn_tile_q)
constexpr int ATTN_K = 32;                       // rows of a streamed tile (nabu_self_attn_tile_k)

struct AttnArgs {
  const float *qkv, *o, *lse, *d_o;              // o, lse: outputs of the forward call, inputs of the backward ones
  float *out, *lse_out, *dqkv;
  const int32_t *len;
  int B, T, H, ld;
  float scale;                                   // 1 / sqrt(dk)
  AttnDrop drop;                                 // read by the DROP instantiations only (attn_drop.h)
  AttnWin win;                                   // read by the WIN instantiations only (attn_win.h)
};

// row index of accumulator register r within a 32 x 32 tile, for the half-wave lk
__device__ __forceinline__ int acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

// B operand from memory: row[2 s + lk] for s < DK / 2
template <int DK>
__device__ __forceinline__ void load_b_operand(const float *row, int lk, float (&reg)[DK / 2]) {
#pragma unroll
  for (int i = 0; i < DK / 4; ++i) {
    const float4 v = *reinterpret_cast<const float4 *>(row + 4 * i);
    reg[2 * i] = lk ? v.y : v.x;
    reg[2 * i + 1] = lk ? v.w : v.z;
  }
}

// One 32-row x DK tile on its way from memory to LDS: 16-byte pieces, piece idx = tid + 256 j is (row idx / (DK / 4),
// columns 4 (idx % (DK / 4))).  Rows at or past `rows` are zeros.
template <int DK>
struct TileRegs {
  static constexpr int NP = ATTN_K * (DK / 4) / 256;   // pieces per thread: 2 (dk 64) or 1 (dk 32)
  float4 v[NP];
  __device__ __forceinline__ void load(const float *base, int ld, int rows, int tid) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int idx = tid + 256 * j, row = idx / (DK / 4), c = 4 * (idx % (DK / 4));
      v[j] = row < rows ? *reinterpret_cast<const float4 *>(base + (size_t)row * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void store(float *tile, int tid) const {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int idx = tid + 256 * j, row = idx / (DK / 4), c = 4 * (idx % (DK / 4));
      float *d = tile + row * (DK + 1) + c;
      d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
    }
  }
};

// acc += Tile Reg^T: M = the tile's 32 rows, N = the wave's 32 rows, reduction over DK
template <int DK>
__device__ __forceinline__ f32x16 tile_times_regs(const float *tile, const float (&reg)[DK / 2], int li, int lk) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float *a = tile + li * (DK + 1) + lk;
#pragma unroll
  for (int s = 0; s < DK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], reg[s], acc, 0, 0, 0);
  return acc;
}

// acc[blk] += Tile^T P: M = 32 columns of the tile per block, N = the wave's 32 rows, reduction over the tile's rows in
// the accumulator's own order (register r of p: rows kappa(r) and kappa(r) + 4)
template <int DK>
__device__ __forceinline__ void tile_t_times_acc(const float *tile, const float (&p)[16], f32x16 (&acc)[DK / 32], int li,
                                                 int lk) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float *a = tile + acc_row(r, lk) * (DK + 1) + li;
#pragma unroll
    for (int blk = 0; blk < DK / 32; ++blk)
      acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[32 * blk], p[r], acc[blk], 0, 0, 0);
  }
}

// a transposed accumulator (lane = row `row` of the output, registers = columns) to memory: 16-byte pieces; row < 0: zeros
template <int DK>
__device__ __forceinline__ void store_acc_t(float *dst, const f32x16 (&acc)[DK / 32], float mul, bool zero, int lk) {
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!zero) v = make_float4(acc[blk][4 * g] * mul, acc[blk][4 * g + 1] * mul, acc[blk][4 * g + 2] * mul, acc[blk][4 * g + 3] * mul);
      *reinterpret_cast<float4 *>(dst + 32 * blk + 8 * g + 4 * lk) = v;
    }
}

template <int DK, bool DROP, bool WIN>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  constexpr int TILE = ATTN_K * (DK + 1);
  __shared__ float Ks[2][TILE], Vs[2][TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * ATTN_Q;
  const int D = a.H * DK;
  const int len = min(max(a.len[b], 0), a.T);
  const int qi = q0 + w * 32 + li;                           // this lane's query
  float *orow = a.out + ((size_t)b * a.T + qi) * D + h * DK;
  float *lse_p = a.lse_out + ((size_t)b * a.H + h) * a.T + qi;
  f32x16 oacc[DK / 32];
  if (q0 >= len) {                                           // a tile of padding frames: zeros, nothing else
    if (qi < a.T) {
      store_acc_t<DK>(orow, oacc, 0.f, true, lk);
      if (lk == 0) *lse_p = 0.f;
    }
    return;
  }
  const float *base = a.qkv + (size_t)b * a.T * a.ld + h * DK;
  float qreg[DK / 2];
  load_b_operand<DK>(base + (size_t)min(qi, len - 1) * a.ld, lk, qreg);   // rows past len: a valid row, dropped at the store
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[blk][r] = 0.f;
  float m = -FLT_MAX, l = 0.f;

  TileRegs<DK> kr, vr;
  int first = 0, ntiles = (len + ATTN_K - 1) / ATTN_K;   // depend on len[b] (and the window) only, never on T
  WinSpan see = {};                                          // WIN: the keys this lane's query sees
  if constexpr (WIN) {                                       // the tiles from lo(first query) to hi(last query below len)
    see = win_keys(a.win, min(qi, len - 1), len);
    first = win_keys(a.win, q0, len).start / ATTN_K;
    ntiles = (win_keys(a.win, min(q0 + ATTN_Q, len) - 1, len).end() + ATTN_K - 1) / ATTN_K;
  }
  auto sees = [&](int k) { if constexpr (WIN) return see.has(k); else return k < len; };
  kr.load(base + D + (size_t)first * ATTN_K * a.ld, a.ld, len - first * ATTN_K, tid);
  vr.load(base + 2 * D + (size_t)first * ATTN_K * a.ld, a.ld, len - first * ATTN_K, tid);
  kr.store(Ks[0], tid);
  vr.store(Vs[0], tid);
  __syncthreads();
  for (int it = first; it < ntiles; ++it) {
    const int k0 = it * ATTN_K, cur = (it - first) & 1;
    const bool more = it + 1 < ntiles;
    if (more) {
      kr.load(base + D + (size_t)(k0 + ATTN_K) * a.ld, a.ld, len - k0 - ATTN_K, tid);
      vr.load(base + 2 * D + (size_t)(k0 + ATTN_K) * a.ld, a.ld, len - k0 - ATTN_K, tid);
    }
    unsigned kept = 0;                                       // DROP: made here, ahead of the S product it is independent of
    if constexpr (DROP) kept = attn_keep16_query(a.drop, b * a.H + h, qi, k0, lk);
    const f32x16 s = tile_times_regs<DK>(Ks[cur], qreg, li, lk);
    float p[16], mt = -FLT_MAX;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = s[r] * a.scale;
      if (sees(k0 + acc_row(r, lk))) mt = fmaxf(mt, p[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float mn = fmaxf(m, mt);
    const float alpha = expf(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = sees(k0 + acc_row(r, lk)) ? expf(p[r] - mn) : 0.f;
      ps += p[r];                                            // the undropped probability
      if constexpr (DROP) p[r] *= attn_drop_scale(a.drop, kept, r);
    }
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[blk][r] *= alpha;    // the one rescale of this key tile
    tile_t_times_acc<DK>(Vs[cur], p, oacc, li, lk);
    if (more) {
      kr.store(Ks[cur ^ 1], tid);
      vr.store(Vs[cur ^ 1], tid);
    }
    __syncthreads();
  }
  if (qi >= a.T) return;
  const bool pad = qi >= len;
  store_acc_t<DK>(orow, oacc, 1.f / l, pad, lk);
  if (lk == 0) *lse_p = pad ? 0.f : m + logf(l);
}

template <int DK, bool DROP, bool WIN>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(AttnArgs a) {
  constexpr int TILE = ATTN_K * (DK + 1);
  __shared__ float Ks[2][TILE], Vs[2][TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * ATTN_Q;
  const int D = a.H * DK;
  const int len = min(max(a.len[b], 0), a.T);
  const int qi = q0 + w * 32 + li;
  float *dqrow = a.dqkv + ((size_t)b * a.T + qi) * a.ld + h * DK;
  f32x16 dq[DK / 32];
  if (q0 >= len) {
    if (qi < a.T) store_acc_t<DK>(dqrow, dq, 0.f, true, lk);
    return;
  }
  const int qc = min(qi, len - 1);
  const float *base = a.qkv + (size_t)b * a.T * a.ld + h * DK;
  float qreg[DK / 2], doreg[DK / 2];
  load_b_operand<DK>(base + (size_t)qc * a.ld, lk, qreg);
  load_b_operand<DK>(a.d_o + ((size_t)b * a.T + qc) * D + h * DK, lk, doreg);
  float delta = 0.f;
  {                                                          // delta = rowsum(dO . O): this lane's half, then the other's
    float oreg[DK / 2];
    load_b_operand<DK>(a.o + ((size_t)b * a.T + qc) * D + h * DK, lk, oreg);
#pragma unroll
    for (int s = 0; s < DK / 2; ++s) delta = fmaf(doreg[s], oreg[s], delta);
    delta += __shfl_xor(delta, 32);
  }
  const float lse = a.lse[((size_t)b * a.H + h) * a.T + qc];
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[blk][r] = 0.f;

  TileRegs<DK> kr, vr;
  int first = 0, ntiles = (len + ATTN_K - 1) / ATTN_K;
  WinSpan see = {};                                          // WIN: the keys this lane's query sees
  if constexpr (WIN) {                                       // the tiles from lo(first query) to hi(last query below len)
    see = win_keys(a.win, min(qi, len - 1), len);
    first = win_keys(a.win, q0, len).start / ATTN_K;
    ntiles = (win_keys(a.win, min(q0 + ATTN_Q, len) - 1, len).end() + ATTN_K - 1) / ATTN_K;
  }
  auto sees = [&](int k) { if constexpr (WIN) return see.has(k); else return k < len; };
  kr.load(base + D + (size_t)first * ATTN_K * a.ld, a.ld, len - first * ATTN_K, tid);
  vr.load(base + 2 * D + (size_t)first * ATTN_K * a.ld, a.ld, len - first * ATTN_K, tid);
  kr.store(Ks[0], tid);
  vr.store(Vs[0], tid);
  __syncthreads();
  for (int it = first; it < ntiles; ++it) {
    const int k0 = it * ATTN_K, cur = (it - first) & 1;
    const bool more = it + 1 < ntiles;
    if (more) {
      kr.load(base + D + (size_t)(k0 + ATTN_K) * a.ld, a.ld, len - k0 - ATTN_K, tid);
      vr.load(base + 2 * D + (size_t)(k0 + ATTN_K) * a.ld, a.ld, len - k0 - ATTN_K, tid);
    }
    unsigned kept = 0;
    if constexpr (DROP) kept = attn_keep16_query(a.drop, b * a.H + h, qi, k0, lk);
    const f32x16 s = tile_times_regs<DK>(Ks[cur], qreg, li, lk);
    const f32x16 dp = tile_times_regs<DK>(Vs[cur], doreg, li, lk);
    float ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = sees(k0 + acc_row(r, lk)) ? expf(s[r] * a.scale - lse) : 0.f;
      if constexpr (DROP) ds[r] = p * (dp[r] * attn_drop_scale(a.drop, kept, r) - delta);   // dP = d . (dO V^T)
      else ds[r] = p * (dp[r] - delta);
    }
    tile_t_times_acc<DK>(Ks[cur], ds, dq, li, lk);
    if (more) {
      kr.store(Ks[cur ^ 1], tid);
      vr.store(Vs[cur ^ 1], tid);
    }
    __syncthreads();
  }
  if (qi < a.T) store_acc_t<DK>(dqrow, dq, a.scale, qi >= len, lk);
}

template <int DK, bool DROP, bool WIN>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(AttnArgs a) {
  constexpr int TILE = ATTN_K * (DK + 1);
  constexpr int PPR = DK / 4;                                // 16-byte pieces per row
  __shared__ float Qs[2][TILE], dOs[2][TILE], lse_s[2][ATTN_K], delta_s[2][ATTN_K];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * ATTN_Q;
  const int D = a.H * DK;
  const int len = min(max(a.len[b], 0), a.T);
  const int ki = k0 + w * 32 + li;                           // this lane's key
  float *dkrow = a.dqkv + ((size_t)b * a.T + ki) * a.ld + D + h * DK;
  f32x16 dk[DK / 32], dv[DK / 32];
  if (k0 >= len) {
    if (ki < a.T) {
      store_acc_t<DK>(dkrow, dk, 0.f, true, lk);
      store_acc_t<DK>(dkrow + D, dv, 0.f, true, lk);
    }
    return;
  }
  const float *base = a.qkv + (size_t)b * a.T * a.ld + h * DK;
  const float *obase = a.o + (size_t)b * a.T * D + h * DK, *dobase = a.d_o + (size_t)b * a.T * D + h * DK;
  const float *lse = a.lse + ((size_t)b * a.H + h) * a.T;
  const bool kvalid = ki < len;
  float kreg[DK / 2], vreg[DK / 2];
  load_b_operand<DK>(base + D + (size_t)min(ki, len - 1) * a.ld, lk, kreg);
  load_b_operand<DK>(base + 2 * D + (size_t)min(ki, len - 1) * a.ld, lk, vreg);
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[blk][r] = dv[blk][r] = 0.f;

  TileRegs<DK> qr, dor;
  float dpart[TileRegs<DK>::NP], lse_r = 0.f;
  auto gload = [&](int t0) {                                 // Q, dO, delta's pieces (from dO and O) and lse of queries t0 .. t0 + 31
    qr.load(base + (size_t)t0 * a.ld, a.ld, len - t0, tid);
    dor.load(dobase + (size_t)t0 * D, D, len - t0, tid);
    TileRegs<DK> orr;
    orr.load(obase + (size_t)t0 * D, D, len - t0, tid);
#pragma unroll
    for (int j = 0; j < TileRegs<DK>::NP; ++j) {
      float d = dor.v[j].x * orr.v[j].x;
      d = fmaf(dor.v[j].y, orr.v[j].y, d); d = fmaf(dor.v[j].z, orr.v[j].z, d); d = fmaf(dor.v[j].w, orr.v[j].w, d);
#pragma unroll
      for (int o = PPR / 2; o >= 1; o >>= 1) d += __shfl_xor(d, o);    // the PPR lanes of a row: every lane gets the sum
      dpart[j] = d;
    }
    if (tid < ATTN_K) lse_r = t0 + tid < len ? lse[t0 + tid] : 0.f;
  };
  auto sstore = [&](int buf) {
    qr.store(Qs[buf], tid);
    dor.store(dOs[buf], tid);
#pragma unroll
    for (int j = 0; j < TileRegs<DK>::NP; ++j) {
      const int idx = tid + 256 * j;
      if (idx % PPR == 0) delta_s[buf][idx / PPR] = dpart[j];
    }
    if (tid < ATTN_K) lse_s[buf][tid] = lse_r;
  };

  int first = 0, ntiles = (len + ATTN_K - 1) / ATTN_K;
  WinSpan seen = {};                                         // WIN: the queries that see this lane's key (none past len)
  if constexpr (WIN) {                                       // the query tiles from qlo(first key) to qhi(last key below len)
    seen = win_queries(a.win, min(ki, len - 1), len);
    if (!kvalid) seen.span = 0;
    first = win_queries(a.win, k0, len).start / ATTN_K;
    ntiles = (win_queries(a.win, min(k0 + ATTN_Q, len) - 1, len).end() + ATTN_K - 1) / ATTN_K;
  }
  auto seen_by = [&](int q) { if constexpr (WIN) return seen.has(q); else return kvalid && q < len; };
  gload(first * ATTN_K);
  sstore(0);
  __syncthreads();
  for (int it = first; it < ntiles; ++it) {
    const int t0 = it * ATTN_K, cur = (it - first) & 1;
    const bool more = it + 1 < ntiles;
    if (more) gload(t0 + ATTN_K);
    unsigned kept = 0;
    if constexpr (DROP) kept = attn_keep16_key(a.drop, b * a.H + h, t0, ki, lk, lane);
    const f32x16 s = tile_times_regs<DK>(Qs[cur], kreg, li, lk);       // S = Q K^T: lane = key, registers = queries
    const f32x16 dp = tile_times_regs<DK>(dOs[cur], vreg, li, lk);     // dP = dO V^T
    float p[16], ds[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = acc_row(r, lk);
      p[r] = seen_by(t0 + qq) ? expf(s[r] * a.scale - lse_s[cur][qq]) : 0.f;
      if constexpr (DROP) {                                            // dS keeps the undropped P; dV takes d . P
        const float d = attn_drop_scale(a.drop, kept, r);
        ds[r] = p[r] * (dp[r] * d - delta_s[cur][qq]);
        p[r] *= d;
      } else {
        ds[r] = p[r] * (dp[r] - delta_s[cur][qq]);
      }
    }
    tile_t_times_acc<DK>(dOs[cur], p, dv, li, lk);                     // dV^T = dO^T P
    tile_t_times_acc<DK>(Qs[cur], ds, dk, li, lk);                     // dK^T = Q^T dS
    if (more) sstore(cur ^ 1);
    __syncthreads();
  }
  if (ki >= a.T) return;
  store_acc_t<DK>(dkrow, dk, a.scale, !kvalid, lk);
  store_acc_t<DK>(dkrow + D, dv, 1.f, !kvalid, lk);
}

// x[b, t, :] += pe[t, :] for t < len[b]
__global__ __launch_bounds__(256) void add_positions_kernel(int B, int T, int D, float *x, const float *pe,
                                                             const int32_t *len) {
  const size_t total = (size_t)B * T * D;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i / D % T), b = (int)(i / ((size_t)D * T));
    if (t < len[b]) x[i] += pe[(size_t)t * D + i % D];
  }
}

static bool attn_al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int attn_shape(const char *what, int B, int T, int H, int dk, int ld) {
  NABU_CHECK_ARG(B >= 0 && T >= 0, "%s: negative batch or time dimension", what);
  NABU_CHECK_ARG(dk == 32 || dk == 64, "%s: head width dk = %d, must be 32 or 64", what, dk);
  NABU_CHECK_ARG(H >= 1 && H * dk <= 1024, "%s: H = %d heads of width %d: D = H dk must be in dk..1024", what, H, dk);
  NABU_CHECK_ARG(ld >= 3 * H * dk, "%s: ld = %d < 3 D = %d", what, ld, 3 * H * dk);
  NABU_CHECK_ARG(ld % 4 == 0, "%s: ld = %d is not a multiple of 4 (rows are read in 16-byte pieces)", what, ld);
  NABU_CHECK_ARG(B <= 65535, "%s: B = %d > 65535", what, B);
  return 0;
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_self_attn_tile_q(void) { return ATTN_Q; }
extern "C" int nabu_self_attn_tile_k(void) { return ATTN_K; }

// the forward launch of nabu_self_attn_fwd (drop == nullptr, or keep == 1: the plain instantiations), of
// nabu_self_attn_drop_fwd and of nabu_self_attn_win_fwd (win != nullptr: the WIN instantiations, at every C)
static int attn_fwd_launch(const char *what, int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len,
                           const AttnDrop *drop, const AttnWin *win, float *o, float *lse, nabu_stream_t stream) {
  NABU_TRY(attn_shape(what, B, T, H, dk, ld));
  NABU_CHECK_ARG(qkv && len && o && lse, "%s: null pointer", what);
  NABU_CHECK_ARG(attn_al16(qkv) && attn_al16(o), "%s: qkv and o must be 16-byte aligned", what);
  if (B == 0 || T == 0) return 0;
  AttnArgs a = {};
  a.qkv = qkv; a.len = len; a.out = o; a.lse_out = lse;
  a.B = B; a.T = T; a.H = H; a.ld = ld; a.scale = 1.f / sqrtf((float)dk);
  const dim3 grid((T + ATTN_Q - 1) / ATTN_Q, H, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool dropping = drop && drop->keep < 1.f;
  if (dropping) a.drop = *drop;
  if (win) a.win = *win;
  ATTN_LAUNCH(attn_fwd_kernel, dk, dropping, win != nullptr, grid, s, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

static int attn_bwd_launch(const char *what, int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                           const float *lse, const float *d_o, const int32_t *len, const AttnDrop *drop, const AttnWin *win,
                           float *dqkv, nabu_stream_t stream) {
  NABU_TRY(attn_shape(what, B, T, H, dk, ld));
  NABU_CHECK_ARG(qkv && o && lse && d_o && len && dqkv, "%s: null pointer", what);
  NABU_CHECK_ARG(attn_al16(qkv) && attn_al16(o) && attn_al16(d_o) && attn_al16(dqkv),
                 "%s: qkv, o, do and dqkv must be 16-byte aligned", what);
  if (B == 0 || T == 0) return 0;
  AttnArgs a = {};
  a.qkv = qkv; a.o = o; a.lse = lse; a.d_o = d_o; a.len = len; a.dqkv = dqkv;
  a.B = B; a.T = T; a.H = H; a.ld = ld; a.scale = 1.f / sqrtf((float)dk);
  const dim3 grid((T + ATTN_Q - 1) / ATTN_Q, H, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool dropping = drop && drop->keep < 1.f;
  if (dropping) a.drop = *drop;
  if (win) a.win = *win;
  ATTN_LAUNCH(attn_bwd_dkv_kernel, dk, dropping, win != nullptr, grid, s, a);
  ATTN_LAUNCH(attn_bwd_dq_kernel, dk, dropping, win != nullptr, grid, s, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_self_attn_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len, float *o,
                                  float *lse, nabu_stream_t stream) {
  return attn_fwd_launch("self_attn_fwd", B, T, H, dk, qkv, ld, len, nullptr, nullptr, o, lse, stream);
}

extern "C" int nabu_self_attn_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o, const float *lse,
                                  const float *d_o, const int32_t *len, float *dqkv, nabu_stream_t stream) {
  return attn_bwd_launch("self_attn_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, nullptr, nullptr, dqkv, stream);
}

extern "C" int nabu_self_attn_drop_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len, float keep,
                                       unsigned long long seed, unsigned long long offset, float *o, float *lse,
                                       nabu_stream_t stream) {
  AttnDrop d;
  NABU_TRY(attn_drop_args("self_attn_drop_fwd", T, keep, seed, offset, &d));
  return attn_fwd_launch("self_attn_drop_fwd", B, T, H, dk, qkv, ld, len, &d, nullptr, o, lse, stream);
}

extern "C" int nabu_self_attn_drop_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                                       const float *lse, const float *d_o, const int32_t *len, float keep,
                                       unsigned long long seed, unsigned long long offset, float *dqkv,
                                       nabu_stream_t stream) {
  AttnDrop d;
  NABU_TRY(attn_drop_args("self_attn_drop_bwd", T, keep, seed, offset, &d));
  return attn_bwd_launch("self_attn_drop_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, &d, nullptr, dqkv, stream);
}

extern "C" int nabu_self_attn_win_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len, float keep,
                                      unsigned long long seed, unsigned long long offset, int chunk, int left_chunks,
                                      float *o, float *lse, nabu_stream_t stream) {
  AttnDrop d;
  AttnWin w;
  NABU_TRY(attn_drop_args("self_attn_win_fwd", T, keep, seed, offset, &d));
  NABU_TRY(attn_win_args("self_attn_win_fwd", T, chunk, left_chunks, &w));
  return attn_fwd_launch("self_attn_win_fwd", B, T, H, dk, qkv, ld, len, &d, &w, o, lse, stream);
}

extern "C" int nabu_self_attn_win_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                                      const float *lse, const float *d_o, const int32_t *len, float keep,
                                      unsigned long long seed, unsigned long long offset, int chunk, int left_chunks,
                                      float *dqkv, nabu_stream_t stream) {
  AttnDrop d;
  AttnWin w;
  NABU_TRY(attn_drop_args("self_attn_win_bwd", T, keep, seed, offset, &d));
  NABU_TRY(attn_win_args("self_attn_win_bwd", T, chunk, left_chunks, &w));
  return attn_bwd_launch("self_attn_win_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, &d, &w, dqkv, stream);
}

extern "C" int nabu_add_positions_f32(int B, int T, int D, float *x, const float *pe, const int32_t *len,
                                      nabu_stream_t stream) {
  NABU_CHECK_ARG(B >= 0 && T >= 0 && D >= 1, "add_positions: bad dimensions");
  NABU_CHECK_ARG(x && pe && len, "add_positions: null pointer");
  const size_t total = (size_t)B * T * D;
  if (total == 0) return 0;
  hipLaunchKernelGGL(add_positions_kernel, dim3((unsigned)min((total + 255) / 256, (size_t)8192)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), B, T, D, x, pe, len);
  NABU_LAUNCH_CHECK();
  return 0;
}
