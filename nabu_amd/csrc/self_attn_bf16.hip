// self_attn_bf16.hip — the self-attention of self_attn.hip with its four matrix products on the bf16 matrix pipe
// (v_mfma_f32_32x32x16_bf16, eight times the reduction depth of v_mfma_f32_32x32x2_f32 per instruction); selected by
// attention_precision = bf16.  Same operands, same contract (include/nabu_hip.h): qkv, o, lse, do and dqkv are fp32 in
// memory; the T x T score matrix exists only as accumulator registers.
//
// WHERE THE 16-BIT ROUNDINGS ARE (round to nearest even, v_cvt_pk_bf16_f32): Q, K, V and dO when they become matrix
// operands (on the way into LDS or into operand registers); P as the operand of O = P V and dV = P^T dO; dS as the operand
// of dQ and dK.  Everything else is fp32: the accumulators, the 1/sqrt(dk) scale (applied to the fp32 score), the running
// maximum, the running sum (over the UNROUNDED probabilities), the once-per-tile rescale, lse, delta = rowsum(dO . O)
// (from the fp32 dO and O) and the final division.  The exponential is v_exp_f32 of x log2(e): with sixteen exponentials
// per 32 x 32 score tile and a matrix pipe eight times faster, the VALU is what these kernels wait for, and libm's expf
// costs four times as many instructions; its error (1 ulp, plus |x| u from the product) disappears under u16 = 2^-8.
//
// THE LAYOUT (what is kept of self_attn.hip: lane = query, and no probability ever crosses a lane).
//   * A 32x32x16 step takes 8 consecutive reduction indices from each half-wave: the operand fragment of a lane is row
//     lane & 31, chunk lane >> 5 of a [32][16] block — 16 bytes of bf16.  A wave computes S^T = K Q^T (M = keys, N = its own
//     32 queries): the B operand is the lane's query row, rounded once into DK / 16 fragments; the A operand is the K tile
//     in LDS, ROW-MAJOR in bf16, one ds_read_b128 per step.  In the 32 x 32 accumulator a lane holds one query's column:
//     register r of half-wave lk is key kappa(r) + 4 lk, kappa(r) = (r & 3) + 8 (r >> 2).
//   * The accumulator is fed back as the B operand of O^T = V^T P^T.  Step s (0, 1) packs registers 8 s .. 8 s + 7 into
//     four v_cvt_pk_bf16_f32 results: element e of half-wave lk is key 16 s + (e & 3) + 8 (e >> 2) + 4 lk, where the
//     instruction expects reduction index 16 s + 8 lk + e.  That is the key index with bits 2 and 3 swapped, so V is staged
//     TRANSPOSED AND KEY-PERMUTED, [dk][position] in bf16 with position = key with bits 2 and 3 swapped: the 8 values a
//     lane needs are again one ds_read_b128.  O^T's accumulator keeps lane = query, so rescale and division are in-lane.
//   * Backward, queries owned (attn_bf16_bwd_dq_kernel): S^T = K Q^T and dP^T = V dO^T from row-major K and V tiles, dS^T
//     fed back into dQ^T = K^T dS^T against a second, transposed and permuted copy of the K tile.
//   * Backward, keys owned (attn_bf16_bwd_dkv_kernel): K^T and V^T are the B fragments in registers; Q and dO tiles are
//     staged in both layouts (row-major for S = Q K^T and dP = dO V^T, transposed and permuted for dV^T = dO^T P and
//     dK^T = Q^T dS), with lse and delta (from the fp32 dO and O, by the staging threads) beside them.
//
// THE TILES.  A workgroup of four waves owns A16_Q = 128 rows, a wave 32 (nabu_self_attn_bf16_tile_q).  The streamed
// tile is A16_K = 64 rows per barrier (nabu_self_attn_bf16_tile_k), twice self_attn.hip's: the matrix time of a 32-key
// tile fell from 4096 to 256 cycles (dk 64), so barrier, maximum exchange and rescale are no longer hidden behind it; at 64
// keys there is one of each per 64 keys, and the forward kernel still holds S^T (32 registers) and O^T (32) comfortably.
// The backward kernels walk the 64 rows as two halves of 32 to keep S and dP at 16 registers each.  Forward and dQ kernel
// double-buffer their tiles (fetch into registers under the matrix work, store to the other buffer, ONE barrier per
// tile); the dK/dV kernel has four tiles per step and keeps one buffer and two barriers, inside 64 KiB of static LDS.
//
// STAGING AND BANKS.  A thread stages a 4-row x 4-column block (four 16-byte loads, DK / 4 consecutive threads cover a
// 256- or 128-byte row), rounds it, and writes it row-major (4 x 8 bytes) and/or transposed (4 x 8 bytes: the 4 rows are
// 4 consecutive positions, the permutation moves bits 2 and 3 only).  Row strides are (DK + 8) bf16 row-major (144 or
// 80 bytes) and 64 + 8 bf16 transposed (144 bytes).  Checked against the access pattern: a ds_read_b128 is served 8
// lanes at a time, and rows 0..7 at 36 (20) words apart start at banks 0, 4, .. 28 in some order — conflict-free, like the
// 80-byte rows of gemm_bf16.hip; the row-major stores put 16 (8) lanes side by side in one row.  The transposing stores
// are NOT conflict-free (the rows of 16 neighbouring lanes are 4 x 144 bytes apart: two bank groups); they are 4 stores
// per thread and 64-row tile against 32 to 64 fragment reads, and were left so.
// Rows at or past len[b] are staged as zeros, whatever memory holds.  The running maximum starts at -FLT_MAX and a
// masked key is left out by a select: every tile walked has a key below len[b], so no infinity and no NaN is ever made.
// THE WINDOW (the WIN instantiations, nabu_self_attn_bf16_win_*; attn_win.h), as in self_attn.hip with the 64-key tile:
// a lane's interval is computed once in the prologue and tested by one subtract and one unsigned compare per score, in
// both halves of a tile; the walk runs from lo(first query) / 64 to ceil(hi(last query below len) / 64) - 1 (dK/dV: the
// query tiles from qlo(first key) to qhi(last key below len)), boundaries multiples of 64 counted from row 0, the first
// fetch at the first walked tile.  THE INVARIANT that replaces "every tile walked has a key below len": every lane meets
// a key it sees somewhere on the walk (its own), but not in every tile; where it sees none, the tile maximum stays
// -FLT_MAX, m_new = m_old, the rescale is 2^0 = 1 exactly (also while m is still -FLT_MAX), all 32 probabilities are
// selected to +0.0 BEFORE v_cvt_pk_bf16_f32, and l and the accumulators keep their bits.  The backward kernels select
// P = exp(s - lse) to 0 outside the window whatever s is.
// Built with packed fp32 VALU instructions switched off (build.py, as self_attn.hip).
#include <float.h>

#include "attn_drop.h"
#include "attn_win.h"
#include "gemm_args.h"

namespace nabu {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int A16_Q = 128;                       // rows a workgroup owns: four waves x 32 (nabu_self_attn_bf16_tile_q)
constexpr int A16_K = 64;                        // rows of a streamed tile (nabu_self_attn_bf16_tile_k)
constexpr int A16_TS = 2 * (A16_K + 8);          // bytes per row of a transposed tile [DK][64 positions + 8 pad]

template <int DK>
struct A16 {
  static constexpr int RS = 2 * (DK + 8);        // bytes per row of a row-major tile [64][DK + 8 pad]
  static constexpr int ROWS = A16_K * RS;        // bytes of a row-major tile
  static constexpr int COLS = DK * A16_TS;       // bytes of a transposed tile
  static constexpr int PPR = DK / 4;             // 16-byte pieces (and staging threads) per row
  static constexpr int NB = (A16_K / 4) * PPR;   // 4 x 4 blocks per tile: 256 (dk 64) or 128 (dk 32)
};

struct Attn16Args {
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

// two fp32 -> one register of two bf16, round to nearest even (low half = first element)
__device__ __forceinline__ unsigned pack2(float x0, float x1) {
  const f32x2 v = {x0, x1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

__device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// the 8 fp32 of a row that step s of a B fragment takes from half-wave lk: columns 16 s + 8 lk .. + 7
__device__ __forceinline__ void load8(const float *row, int s, int lk, float (&x)[8]) {
  const float4 u = *reinterpret_cast<const float4 *>(row + 16 * s + 8 * lk);
  const float4 v = *reinterpret_cast<const float4 *>(row + 16 * s + 8 * lk + 4);
  x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
}

__device__ __forceinline__ u32x4 pack8(const float (&x)[8]) {
  return u32x4{pack2(x[0], x[1]), pack2(x[2], x[3]), pack2(x[4], x[5]), pack2(x[6], x[7])};
}

// B operand from memory: one row, rounded, as DK / 16 fragments
template <int DK>
__device__ __forceinline__ void load_b_operand(const float *row, int lk, u32x4 (&reg)[DK / 16]) {
#pragma unroll
  for (int s = 0; s < DK / 16; ++s) {
    float x[8];
    load8(row, s, lk, x);
    reg[s] = pack8(x);
  }
}

// B operand from an accumulator: registers 8 s .. 8 s + 7 of x, rounded (keys in the permuted order of the header)
__device__ __forceinline__ u32x4 acc_operand(const float (&x)[16], int s) {
  return u32x4{pack2(x[8 * s], x[8 * s + 1]), pack2(x[8 * s + 2], x[8 * s + 3]), pack2(x[8 * s + 4], x[8 * s + 5]),
               pack2(x[8 * s + 6], x[8 * s + 7])};
}

// One 4-row x 4-column block of a 64-row x DK tile on its way from memory to LDS: thread tid < NB has rows 4 rg .. + 3,
// columns 4 dg .. + 3 with dg = tid % PPR, rg = tid / PPR.  Rounded at the load; kept row-major (ROWS) and/or transposed
// (COLS).  Rows at or past `rows` are zeros.
template <int DK, bool ROWS, bool COLS>
struct Block {
  unsigned r[8], c[8];                         // (the side a kernel does not ask for is never written or read)
  __device__ __forceinline__ void set(const f32x4 (&v)[4]) {
    if constexpr (ROWS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) { r[2 * i] = pack2(v[i][0], v[i][1]); r[2 * i + 1] = pack2(v[i][2], v[i][3]); }
    }
    if constexpr (COLS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[2 * j] = pack2(v[0][j], v[1][j]); c[2 * j + 1] = pack2(v[2][j], v[3][j]); }
    }
  }
  static __device__ __forceinline__ void fetch(const float *base, int ld, int rows, int tid, f32x4 (&v)[4]) {
    const int dg = tid % A16<DK>::PPR, rg = tid / A16<DK>::PPR;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * rg + i;
      v[i] = (tid < A16<DK>::NB && row < rows) ? *reinterpret_cast<const f32x4 *>(base + (size_t)row * ld + 4 * dg)
                                               : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ __forceinline__ void load(const float *base, int ld, int rows, int tid) {
    f32x4 v[4];
    fetch(base, ld, rows, tid, v);
    set(v);
  }
  __device__ __forceinline__ void store(char *rows_tile, char *cols_tile, int tid) const {
    if (tid >= A16<DK>::NB) return;
    const int dg = tid % A16<DK>::PPR, rg = tid / A16<DK>::PPR;
    if constexpr (ROWS) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<u32x2 *>(rows_tile + (4 * rg + i) * A16<DK>::RS + 8 * dg) = u32x2{r[2 * i], r[2 * i + 1]};
    }
    if constexpr (COLS) {
      const int row = 4 * rg, pos = (row & ~12) | ((row & 4) << 1) | ((row & 8) >> 1);     // bits 2 and 3 swapped
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<u32x2 *>(cols_tile + (4 * dg + j) * A16_TS + 2 * pos) = u32x2{c[2 * j], c[2 * j + 1]};
    }
  }
};

// Tile Reg^T: M = 32 rows of a row-major tile (from `tile`), N = the wave's 32 rows, reduction over DK
template <int DK>
__device__ __forceinline__ f32x16 rows_times_regs(const char *tile, const u32x4 (&reg)[DK / 16], int li, int lk) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const char *a = tile + li * A16<DK>::RS + 16 * lk;
#pragma unroll
  for (int s = 0; s < DK / 16; ++s) acc = mfma(*reinterpret_cast<const u32x4 *>(a + 32 * s), reg[s], acc);
  return acc;
}

// acc[blk] += Tile^T X: M = 32 columns of the tile per block (rows of its transposed copy `tile`), N = the wave's 32 rows,
// reduction over rows 32 half .. 32 half + 31 of the tile in the accumulator's own order
template <int DK>
__device__ __forceinline__ void cols_times_acc(const char *tile, int half, const float (&x)[16], f32x16 (&acc)[DK / 32],
                                               int li, int lk) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u32x4 b = acc_operand(x, s);
    const char *a = tile + li * A16_TS + 2 * (32 * half + 16 * s + 8 * lk);
#pragma unroll
    for (int blk = 0; blk < DK / 32; ++blk)
      acc[blk] = mfma(*reinterpret_cast<const u32x4 *>(a + 32 * blk * A16_TS), b, acc[blk]);
  }
}

// a transposed accumulator (lane = row of the output, registers = columns) to memory in 16-byte pieces; zero: +0.0
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
__global__ __launch_bounds__(256) void attn_bf16_fwd_kernel(Attn16Args a) {
  __shared__ __attribute__((aligned(16))) char Ks[2][A16<DK>::ROWS], Vt[2][A16<DK>::COLS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * A16_Q;
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
  u32x4 qreg[DK / 16];
  load_b_operand<DK>(base + (size_t)min(qi, len - 1) * a.ld, lk, qreg);   // rows past len: a valid row, dropped at the store
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[blk][r] = 0.f;
  float m = -FLT_MAX, l = 0.f;

  Block<DK, true, false> kb;
  Block<DK, false, true> vb;
  int first = 0, ntiles = (len + A16_K - 1) / A16_K;         // depend on len[b] (and the window) only, never on T
  WinSpan see = {};                                          // WIN: the keys this lane's query sees
  if constexpr (WIN) {                                       // the tiles from lo(first query) to hi(last query below len)
    see = win_keys(a.win, min(qi, len - 1), len);
    first = win_keys(a.win, q0, len).start / A16_K;
    ntiles = (win_keys(a.win, min(q0 + A16_Q, len) - 1, len).end() + A16_K - 1) / A16_K;
  }
  auto sees = [&](int k) { if constexpr (WIN) return see.has(k); else return k < len; };
  kb.load(base + D + (size_t)first * A16_K * a.ld, a.ld, len - first * A16_K, tid);
  vb.load(base + 2 * D + (size_t)first * A16_K * a.ld, a.ld, len - first * A16_K, tid);
  kb.store(Ks[0], nullptr, tid);
  vb.store(nullptr, Vt[0], tid);
  __syncthreads();
  for (int it = first; it < ntiles; ++it) {
    const int k0 = it * A16_K, cur = (it - first) & 1;
    const bool more = it + 1 < ntiles;
    if (more) {
      kb.load(base + D + (size_t)(k0 + A16_K) * a.ld, a.ld, len - k0 - A16_K, tid);
      vb.load(base + 2 * D + (size_t)(k0 + A16_K) * a.ld, a.ld, len - k0 - A16_K, tid);
    }
    float p[2][16], mt = -FLT_MAX;
    unsigned kept[2] = {0, 0};                               // DROP: eight blocks per lane and 64-key tile, ahead of the S products
    if constexpr (DROP) {
#pragma unroll
      for (int j = 0; j < 2; ++j) kept[j] = attn_keep16_query(a.drop, b * a.H + h, qi, k0 + 32 * j, lk);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const f32x16 s = rows_times_regs<DK>(Ks[cur] + 32 * j * A16<DK>::RS, qreg, li, lk);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[j][r] = s[r] * a.scale;
        if (sees(k0 + 32 * j + acc_row(r, lk))) mt = fmaxf(mt, p[j][r]);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float mn = fmaxf(m, mt);
    const float alpha = exp_fast(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[j][r] = sees(k0 + 32 * j + acc_row(r, lk)) ? exp_fast(p[j][r] - mn) : 0.f;
        ps += p[j][r];                                       // the unrounded, undropped probability
        if constexpr (DROP) p[j][r] *= attn_drop_scale(a.drop, kept[j], r);     // in fp32, before the rounding
      }
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[blk][r] *= alpha;    // the one rescale of this key tile
#pragma unroll
    for (int j = 0; j < 2; ++j) cols_times_acc<DK>(Vt[cur], j, p[j], oacc, li, lk);
    if (more) {
      kb.store(Ks[cur ^ 1], nullptr, tid);
      vb.store(nullptr, Vt[cur ^ 1], tid);
    }
    __syncthreads();
  }
  if (qi >= a.T) return;
  const bool pad = qi >= len;
  store_acc_t<DK>(orow, oacc, 1.f / l, pad, lk);
  if (lk == 0) *lse_p = pad ? 0.f : m + logf(l);
}

template <int DK, bool DROP, bool WIN>
__global__ __launch_bounds__(256) void attn_bf16_bwd_dq_kernel(Attn16Args a) {
  __shared__ __attribute__((aligned(16))) char Ks[2][A16<DK>::ROWS], Kt[2][A16<DK>::COLS], Vs[2][A16<DK>::ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * A16_Q;
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
  u32x4 qreg[DK / 16], doreg[DK / 16];
  load_b_operand<DK>(base + (size_t)qc * a.ld, lk, qreg);
  float delta = 0.f;
  {                                                          // delta = rowsum(dO . O) from the fp32 values: this lane's half, then the other's
    const float *dorow = a.d_o + ((size_t)b * a.T + qc) * D + h * DK, *ovrow = a.o + ((size_t)b * a.T + qc) * D + h * DK;
#pragma unroll
    for (int s = 0; s < DK / 16; ++s) {
      float x[8], y[8];
      load8(dorow, s, lk, x);
      load8(ovrow, s, lk, y);
#pragma unroll
      for (int e = 0; e < 8; ++e) delta = fmaf(x[e], y[e], delta);
      doreg[s] = pack8(x);
    }
    delta += __shfl_xor(delta, 32);
  }
  const float lse = a.lse[((size_t)b * a.H + h) * a.T + qc];
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[blk][r] = 0.f;

  Block<DK, true, true> kb;
  Block<DK, true, false> vb;
  int first = 0, ntiles = (len + A16_K - 1) / A16_K;
  WinSpan see = {};                                          // WIN: the keys this lane's query sees
  if constexpr (WIN) {                                       // the tiles from lo(first query) to hi(last query below len)
    see = win_keys(a.win, min(qi, len - 1), len);
    first = win_keys(a.win, q0, len).start / A16_K;
    ntiles = (win_keys(a.win, min(q0 + A16_Q, len) - 1, len).end() + A16_K - 1) / A16_K;
  }
  auto sees = [&](int k) { if constexpr (WIN) return see.has(k); else return k < len; };
  kb.load(base + D + (size_t)first * A16_K * a.ld, a.ld, len - first * A16_K, tid);
  vb.load(base + 2 * D + (size_t)first * A16_K * a.ld, a.ld, len - first * A16_K, tid);
  kb.store(Ks[0], Kt[0], tid);
  vb.store(Vs[0], nullptr, tid);
  __syncthreads();
  for (int it = first; it < ntiles; ++it) {
    const int k0 = it * A16_K, cur = (it - first) & 1;
    const bool more = it + 1 < ntiles;
    if (more) {
      kb.load(base + D + (size_t)(k0 + A16_K) * a.ld, a.ld, len - k0 - A16_K, tid);
      vb.load(base + 2 * D + (size_t)(k0 + A16_K) * a.ld, a.ld, len - k0 - A16_K, tid);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned kept = 0;
      if constexpr (DROP) kept = attn_keep16_query(a.drop, b * a.H + h, qi, k0 + 32 * j, lk);
      const f32x16 s = rows_times_regs<DK>(Ks[cur] + 32 * j * A16<DK>::RS, qreg, li, lk);
      const f32x16 dp = rows_times_regs<DK>(Vs[cur] + 32 * j * A16<DK>::RS, doreg, li, lk);
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = sees(k0 + 32 * j + acc_row(r, lk)) ? exp_fast(s[r] * a.scale - lse) : 0.f;
        if constexpr (DROP) ds[r] = p * (dp[r] * attn_drop_scale(a.drop, kept, r) - delta);   // dP = d . (dO V^T), fp32
        else ds[r] = p * (dp[r] - delta);
      }
      cols_times_acc<DK>(Kt[cur], j, ds, dq, li, lk);
    }
    if (more) {
      kb.store(Ks[cur ^ 1], Kt[cur ^ 1], tid);
      vb.store(Vs[cur ^ 1], nullptr, tid);
    }
    __syncthreads();
  }
  if (qi < a.T) store_acc_t<DK>(dqrow, dq, a.scale, qi >= len, lk);
}

template <int DK, bool DROP, bool WIN>
__global__ __launch_bounds__(256) void attn_bf16_bwd_dkv_kernel(Attn16Args a) {
  constexpr int PPR = A16<DK>::PPR;
  __shared__ __attribute__((aligned(16))) char Qs[A16<DK>::ROWS], Qt[A16<DK>::COLS], dOs[A16<DK>::ROWS], dOt[A16<DK>::COLS];
  __shared__ float lse_s[A16_K], delta_s[A16_K];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * A16_Q;
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
  u32x4 kreg[DK / 16], vreg[DK / 16];
  load_b_operand<DK>(base + D + (size_t)min(ki, len - 1) * a.ld, lk, kreg);
  load_b_operand<DK>(base + 2 * D + (size_t)min(ki, len - 1) * a.ld, lk, vreg);
#pragma unroll
  for (int blk = 0; blk < DK / 32; ++blk)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[blk][r] = dv[blk][r] = 0.f;

  Block<DK, true, true> qb, dob;
  float dpart[4], lse_r = 0.f;
  auto gload = [&](int t0) {                                 // Q, dO, delta's pieces (from the fp32 dO and O) and lse of queries t0 .. t0 + 63
    qb.load(base + (size_t)t0 * a.ld, a.ld, len - t0, tid);
    f32x4 x[4], y[4];
    Block<DK, true, true>::fetch(dobase + (size_t)t0 * D, D, len - t0, tid, x);
    Block<DK, true, true>::fetch(obase + (size_t)t0 * D, D, len - t0, tid, y);
    dob.set(x);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float d = x[i][0] * y[i][0];
      d = fmaf(x[i][1], y[i][1], d); d = fmaf(x[i][2], y[i][2], d); d = fmaf(x[i][3], y[i][3], d);
#pragma unroll
      for (int o = PPR / 2; o >= 1; o >>= 1) d += __shfl_xor(d, o);    // the PPR lanes of a row: every lane gets the sum
      dpart[i] = d;
    }
    if (tid < A16_K) lse_r = t0 + tid < len ? lse[t0 + tid] : 0.f;
  };
  auto sstore = [&]() {
    qb.store(Qs, Qt, tid);
    dob.store(dOs, dOt, tid);
    if (tid < A16<DK>::NB && tid % PPR == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) delta_s[4 * (tid / PPR) + i] = dpart[i];
    }
    if (tid < A16_K) lse_s[tid] = lse_r;
  };

  int first = 0, ntiles = (len + A16_K - 1) / A16_K;
  WinSpan seen = {};                                         // WIN: the queries that see this lane's key (none past len)
  if constexpr (WIN) {                                       // the query tiles from qlo(first key) to qhi(last key below len)
    seen = win_queries(a.win, min(ki, len - 1), len);
    if (!kvalid) seen.span = 0;
    first = win_queries(a.win, k0, len).start / A16_K;
    ntiles = (win_queries(a.win, min(k0 + A16_Q, len) - 1, len).end() + A16_K - 1) / A16_K;
  }
  auto seen_by = [&](int q) { if constexpr (WIN) return seen.has(q); else return kvalid && q < len; };
  gload(first * A16_K);
  for (int it = first; it < ntiles; ++it) {
    const int t0 = it * A16_K;
    sstore();
    __syncthreads();
    if (it + 1 < ntiles) gload(t0 + A16_K);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      unsigned kept = 0;
      if constexpr (DROP) kept = attn_keep16_key(a.drop, b * a.H + h, t0 + 32 * j, ki, lk, lane);
      const f32x16 s = rows_times_regs<DK>(Qs + 32 * j * A16<DK>::RS, kreg, li, lk);       // S = Q K^T: lane = key, registers = queries
      const f32x16 dp = rows_times_regs<DK>(dOs + 32 * j * A16<DK>::RS, vreg, li, lk);     // dP = dO V^T
      float p[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qq = 32 * j + acc_row(r, lk);
        p[r] = seen_by(t0 + qq) ? exp_fast(s[r] * a.scale - lse_s[qq]) : 0.f;
        if constexpr (DROP) {                                  // dS keeps the undropped P; dV takes d . P, rounded after the multiply
          const float d = attn_drop_scale(a.drop, kept, r);
          ds[r] = p[r] * (dp[r] * d - delta_s[qq]);
          p[r] *= d;
        } else {
          ds[r] = p[r] * (dp[r] - delta_s[qq]);
        }
      }
      cols_times_acc<DK>(dOt, j, p, dv, li, lk);                                           // dV^T = dO^T P
      cols_times_acc<DK>(Qt, j, ds, dk, li, lk);                                           // dK^T = Q^T dS
    }
    __syncthreads();                                         // the tile is read; the next one may be stored
  }
  if (ki >= a.T) return;
  store_acc_t<DK>(dkrow, dk, a.scale, !kvalid, lk);
  store_acc_t<DK>(dkrow + D, dv, 1.f, !kvalid, lk);
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int attn_shape(const char *what, int B, int T, int H, int dk, int ld) {
  NABU_CHECK_ARG(B >= 0 && T >= 0, "%s: negative batch or time dimension", what);
  NABU_CHECK_ARG(dk == 32 || dk == 64, "%s: head width dk = %d, must be 32 or 64", what, dk);
  NABU_CHECK_ARG(H >= 1 && H * dk <= 1024, "%s: H = %d heads of width %d: D = H dk must be in dk..1024", what, H, dk);
  NABU_CHECK_ARG(ld >= 3 * H * dk, "%s: ld = %d < 3 D = %d", what, ld, 3 * H * dk);
  NABU_CHECK_ARG(ld % 4 == 0, "%s: ld = %d is not a multiple of 4 (rows are read in 16-byte pieces)", what, ld);
  NABU_CHECK_ARG(B <= 65535, "%s: B = %d > 65535", what, B);
  return 0;
}

}  // namespace
}  // namespace nabu

using namespace nabu;

extern "C" int nabu_self_attn_bf16_tile_q(void) { return A16_Q; }
extern "C" int nabu_self_attn_bf16_tile_k(void) { return A16_K; }

// the forward launch of nabu_self_attn_bf16_fwd (drop == nullptr, or keep == 1: the plain instantiations), of
// nabu_self_attn_bf16_drop_fwd and of nabu_self_attn_bf16_win_fwd (win != nullptr: the WIN instantiations, at every C)
static int attn16_fwd_launch(const char *what, int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len,
                             const AttnDrop *drop, const AttnWin *win, float *o, float *lse, nabu_stream_t stream) {
  NABU_TRY(attn_shape(what, B, T, H, dk, ld));
  NABU_CHECK_ARG(qkv && len && o && lse, "%s: null pointer", what);
  NABU_CHECK_ARG(al16(qkv) && al16(o), "%s: qkv and o must be 16-byte aligned", what);
  if (B == 0 || T == 0) return 0;
  Attn16Args a = {};
  a.qkv = qkv; a.len = len; a.out = o; a.lse_out = lse;
  a.B = B; a.T = T; a.H = H; a.ld = ld; a.scale = 1.f / sqrtf((float)dk);
  const dim3 grid((T + A16_Q - 1) / A16_Q, H, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool dropping = drop && drop->keep < 1.f;
  if (dropping) a.drop = *drop;
  if (win) a.win = *win;
  ATTN_LAUNCH(attn_bf16_fwd_kernel, dk, dropping, win != nullptr, grid, s, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

static int attn16_bwd_launch(const char *what, int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                             const float *lse, const float *d_o, const int32_t *len, const AttnDrop *drop,
                             const AttnWin *win, float *dqkv, nabu_stream_t stream) {
  NABU_TRY(attn_shape(what, B, T, H, dk, ld));
  NABU_CHECK_ARG(qkv && o && lse && d_o && len && dqkv, "%s: null pointer", what);
  NABU_CHECK_ARG(al16(qkv) && al16(o) && al16(d_o) && al16(dqkv), "%s: qkv, o, do and dqkv must be 16-byte aligned", what);
  if (B == 0 || T == 0) return 0;
  Attn16Args a = {};
  a.qkv = qkv; a.o = o; a.lse = lse; a.d_o = d_o; a.len = len; a.dqkv = dqkv;
  a.B = B; a.T = T; a.H = H; a.ld = ld; a.scale = 1.f / sqrtf((float)dk);
  const dim3 grid((T + A16_Q - 1) / A16_Q, H, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool dropping = drop && drop->keep < 1.f;
  if (dropping) a.drop = *drop;
  if (win) a.win = *win;
  ATTN_LAUNCH(attn_bf16_bwd_dkv_kernel, dk, dropping, win != nullptr, grid, s, a);
  ATTN_LAUNCH(attn_bf16_bwd_dq_kernel, dk, dropping, win != nullptr, grid, s, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_self_attn_bf16_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len, float *o,
                                       float *lse, nabu_stream_t stream) {
  return attn16_fwd_launch("self_attn_bf16_fwd", B, T, H, dk, qkv, ld, len, nullptr, nullptr, o, lse, stream);
}

extern "C" int nabu_self_attn_bf16_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                                       const float *lse, const float *d_o, const int32_t *len, float *dqkv,
                                       nabu_stream_t stream) {
  return attn16_bwd_launch("self_attn_bf16_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, nullptr, nullptr, dqkv, stream);
}

extern "C" int nabu_self_attn_bf16_drop_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len,
                                            float keep, unsigned long long seed, unsigned long long offset, float *o,
                                            float *lse, nabu_stream_t stream) {
  AttnDrop d;
  NABU_TRY(attn_drop_args("self_attn_bf16_drop_fwd", T, keep, seed, offset, &d));
  return attn16_fwd_launch("self_attn_bf16_drop_fwd", B, T, H, dk, qkv, ld, len, &d, nullptr, o, lse, stream);
}

extern "C" int nabu_self_attn_bf16_drop_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                                            const float *lse, const float *d_o, const int32_t *len, float keep,
                                            unsigned long long seed, unsigned long long offset, float *dqkv,
                                            nabu_stream_t stream) {
  AttnDrop d;
  NABU_TRY(attn_drop_args("self_attn_bf16_drop_bwd", T, keep, seed, offset, &d));
  return attn16_bwd_launch("self_attn_bf16_drop_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, &d, nullptr, dqkv, stream);
}

extern "C" int nabu_self_attn_bf16_win_fwd(int B, int T, int H, int dk, const float *qkv, int ld, const int32_t *len,
                                           float keep, unsigned long long seed, unsigned long long offset, int chunk,
                                           int left_chunks, float *o, float *lse, nabu_stream_t stream) {
  AttnDrop d;
  AttnWin w;
  NABU_TRY(attn_drop_args("self_attn_bf16_win_fwd", T, keep, seed, offset, &d));
  NABU_TRY(attn_win_args("self_attn_bf16_win_fwd", T, chunk, left_chunks, &w));
  return attn16_fwd_launch("self_attn_bf16_win_fwd", B, T, H, dk, qkv, ld, len, &d, &w, o, lse, stream);
}

extern "C" int nabu_self_attn_bf16_win_bwd(int B, int T, int H, int dk, const float *qkv, int ld, const float *o,
                                           const float *lse, const float *d_o, const int32_t *len, float keep,
                                           unsigned long long seed, unsigned long long offset, int chunk, int left_chunks,
                                           float *dqkv, nabu_stream_t stream) {
  AttnDrop d;
  AttnWin w;
  NABU_TRY(attn_drop_args("self_attn_bf16_win_bwd", T, keep, seed, offset, &d));
  NABU_TRY(attn_win_args("self_attn_bf16_win_bwd", T, chunk, left_chunks, &w));
  return attn16_bwd_launch("self_attn_bf16_win_bwd", B, T, H, dk, qkv, ld, o, lse, d_o, len, &d, &w, dqkv, stream);
}
