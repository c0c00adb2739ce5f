// linear_narrow.hip — a linear layer with a NARROW output (N <= 64 columns: the DNNDecoder's outlayer, [B*T, F] -> 40
// classes) in exact fp32 on v_mfma_f32_16x16x4_f32.
//
// The 128-wide tiles of gemm.hip spend two thirds of their matrix work on columns that do not exist at N = 40, put a
// handful of workgroups on the device and need split-K with a reduce launch to get even those; the layer's four
// products were seven dependent launches.  Here:
//
//   forward   C[M,N] = alpha * A[M,K]·B[K,N] + bias         one launch, a workgroup per 16 rows over the whole K
//   backward  dx = dy·W^T, dW = x^T·dy, db = colsum(dy)      one pass over x and dy + one small reduce launch
//
// Forward: the eight waves of a workgroup take an eighth (32 k) of every 256-k chunk each; B's chunk goes through LDS,
// every lane's A loads are 16 bytes and requested a whole pass of 1024 k ahead, the next chunk of B is in registers
// under the current chunk's MFMAs.  The eight partial tiles are added in wave order at the end.  A row's sum therefore
// has ONE k order — by chunk, by k inside the wave's eighth, then over the eight eighths — whatever rows share its
// workgroup; nothing is handed between workgroups.
//
// Backward: workgroup (ks, rb) owns the 64-k slice ks of a contiguous block rb of rows, so x is read once and dx written
// once over the whole grid (dy, 40 columns, is re-read from L2 by the slices).  A wave owns 16 k of the slice: it keeps
// its 16 x N piece of W in registers (the A operand of dx^T = W·dy^T: a lane ends up with four consecutive k of one row,
// a 16-byte store) and accumulates its 16 x N piece of the block's dW partial in registers over all rows of the block.
// The partials go to a slab [row blocks][K*N + N] (db behind dW, from the ks = 0 workgroups); the reduce launch adds the
// slabs in block order: fixed order, bitwise repeatable, no float atomics.  Slicing K as well as the rows keeps the
// slab at 32 x 164 KB for cfg2 instead of one K x N partial per workgroup of the device.
#include "gemm_args.h"

namespace nabu {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LN_MAXN = 64;
constexpr int LN_ROWS = 16;           // rows of a row tile (the MFMA's 16)
constexpr int LN_KC = 256;            // forward: k-chunk of B in LDS (LN_FW waves x LN_KW k)
constexpr int LN_FW = 8;              // ... waves of a workgroup
constexpr int LN_FT = 64 * LN_FW;     // ... threads
constexpr int LN_KW = LN_KC / LN_FW;  // ... a wave's k of a chunk: two groups of 16
constexpr int LN_PASS = 1024;         // ... k whose A rows a workgroup requests at once (8 x 16 bytes per lane)
constexpr int LN_SUPER = 8;           // backward: row tiles whose x and dy rows a workgroup requests at once
constexpr int LN_LDB = 68;            // 4 * 68 % 32 == 16: the rows k and k + 4 of one ds_read_b32 half hit disjoint banks
constexpr int LN_KS = 64;             // backward: k-slice of a workgroup (4 waves x 16 k)
constexpr int LN_LDX = 80;            // x tile [16 rows][64 k]: rows r and r + 1 of one half 16 banks apart
constexpr int LN_LDD = 66;            // dy tile [16 rows][64 n]: 2 i + q distinct for the dx operand read
constexpr int LN_TARGET_WGS = 512;    // backward grid: one wave of workgroups on a whole MI355X, two per CU

struct LinFwdArgs {
  const float *A, *B, *bias;
  float *C;
  int M, N, K, lda, ldb, ldc;
  float alpha;
  int vecB;      // 16-byte loads of B rows (N % 4 == 0, ldb % 4 == 0)
};

// 250 workgroups at cfg2, one per CU, so nothing hides a workgroup's own waits: the A rows of a whole pass of
// LN_PASS = 1024 k are requested at once (8 x 16 bytes per lane, 64 KB per workgroup), and the B chunk after the
// current one is in registers before the current one is multiplied.
// NT = column tiles of 16, a template parameter: with a run-time bound hipcc puts a branch around every MFMA, and each
// operand read is then issued, waited for and consumed alone — ~350 cycles per MFMA, 34 us at cfg2 where this takes 14
// (LABNOTES.md section 29)
template <int NT>
__global__ __launch_bounds__(LN_FT) void linear_narrow_fwd_kernel(LinFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Bs[];            // [LN_KC][LN_LDB]; the waves' partial tiles afterwards
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int row0 = blockIdx.x * LN_ROWS;
  // lane (li, lq) holds A[row li][k = 4 lq + c] of the 16 k an MFMA step c takes a quad out of
  const float *arow = a.A + (size_t)min(row0 + li, a.M - 1) * a.lda + LN_KW * w + 4 * lq;   // surplus rows: dropped at the store

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 an[LN_PASS / LN_KC][LN_KW / 16];
  float bn[LN_KC * 64 / LN_FT];
#define LN_LOAD_B(kc_)                                                                                            \
  {                                                                                                               \
    if (a.vecB) {                                                                                                 \
      _Pragma("unroll") for (int i = 0; i < LN_KC * 16 / LN_FT; ++i) {                                                    \
        const int idx = tid + LN_FT * i, k = (kc_) + (idx >> 4), c = 4 * (idx & 15);                                \
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                                                               \
        if (k < a.K && c < a.N) v = *reinterpret_cast<const float4 *>(a.B + (size_t)k * a.ldb + c);               \
        bn[4 * i] = v.x; bn[4 * i + 1] = v.y; bn[4 * i + 2] = v.z; bn[4 * i + 3] = v.w;                           \
      }                                                                                                           \
    } else {                                                                                                      \
      _Pragma("unroll") for (int i = 0; i < LN_KC * 64 / LN_FT; ++i) {                                                     \
        const int idx = tid + LN_FT * i, k = (kc_) + (idx >> 6), c = idx & 63;                                      \
        bn[i] = (k < a.K && c < a.N) ? a.B[(size_t)k * a.ldb + c] : 0.f;                                          \
      }                                                                                                           \
    }                                                                                                             \
  }

  LN_LOAD_B(0);
  for (int kp = 0; kp < a.K; kp += LN_PASS) {
#pragma unroll
    for (int ch = 0; ch < LN_PASS / LN_KC; ++ch)
#pragma unroll
      for (int g = 0; g < LN_KW / 16; ++g) {
        const int off = kp + LN_KC * ch + 16 * g;                  // + LN_KW w + 4 lq: this lane's k
        an[ch][g] = off + LN_KW * w + 4 * lq < a.K ? *reinterpret_cast<const float4 *>(arow + off)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
    for (int ch = 0; ch < LN_PASS / LN_KC; ++ch) {
      const int kc = kp + LN_KC * ch;
      if (kc >= a.K) break;                              // uniform over the workgroup
      if (a.vecB) {
#pragma unroll
        for (int i = 0; i < LN_KC * 16 / LN_FT; ++i) {
          const int idx = tid + LN_FT * i;
          *reinterpret_cast<float4 *>(&Bs[(idx >> 4) * LN_LDB + 4 * (idx & 15)]) =
              make_float4(bn[4 * i], bn[4 * i + 1], bn[4 * i + 2], bn[4 * i + 3]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < LN_KC * 64 / LN_FT; ++i) {
          const int idx = tid + LN_FT * i;
          Bs[(idx >> 6) * LN_LDB + (idx & 63)] = bn[i];
        }
      }
      __syncthreads();
      if (kc + LN_KC < a.K) LN_LOAD_B(kc + LN_KC);
#pragma unroll
      for (int g = 0; g < LN_KW / 16; ++g) {
        const int kb = LN_KW * w + 16 * g;
        if (kc + kb >= a.K) break;                       // wave-uniform: nothing but zeros from here on
        const float avs[4] = {an[ch][g].x, an[ch][g].y, an[ch][g].z, an[ch][g].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float *bp = &Bs[(kb + 4 * lq + c) * LN_LDB + li];
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(avs[c], bp[16 * t], acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
#undef LN_LOAD_B

  // the waves' partial tiles, added in wave order: lane holds column 16 t + li, rows 4 lq + r
  float *red = Bs;                                     // [LN_FW][16][64]
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[(w * LN_ROWS + 4 * lq + r) * 64 + 16 * t + li] = acc[t][r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LN_ROWS * 64 / LN_FT; ++i) {
    const int idx = tid + LN_FT * i, r = idx >> 6, c = idx & 63;
    if (c < a.N && row0 + r < a.M) {
      float s = red[idx];
#pragma unroll
      for (int v = 1; v < LN_FW; ++v) s += red[v * LN_ROWS * 64 + idx];
      a.C[(size_t)(row0 + r) * a.ldc + c] = a.alpha * s + (a.bias ? a.bias[c] : 0.f);
    }
  }
}

struct LinBwdArgs {
  const float *x, *dy, *W;
  float *dx, *slab;
  int M, K, N, ldx, ldy, ldw, lddx;
  int rows_per_block;
};

// As in the forward kernel, a workgroup's own waits are what there is to hide:
// the x and dy rows of LN_SUPER = 8 row tiles (128 rows: a whole row block at cfg2) are requested at once, 32 KB of x per
// workgroup and two workgroups per CU, and go through two LDS tile buffers with one barrier per tile.
template <int NT>
__global__ __launch_bounds__(256) void linear_narrow_bwd_kernel(LinBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float Xs[2][LN_ROWS * LN_LDX];
  __shared__ __attribute__((aligned(16))) float Ds[2][LN_ROWS * LN_LDD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int kbase = blockIdx.x * LN_KS, rb = blockIdx.y;
  const int r_begin = rb * a.rows_per_block, r_end = min(a.M, r_begin + a.rows_per_block);
  const size_t slab_len = (size_t)a.K * a.N + a.N;
  float *slab = a.slab + (size_t)rb * slab_len;

  // the wave's 16 k of W as the A operand of dx^T = W·dy^T: lane (li, lq) holds W[k li][n = 4 s + lq] for step s
  // (all 4 NT steps: W and the dy tile hold zeros from N on)
  float wf[4 * NT];
  {
    const int k = kbase + 16 * w + li;
#pragma unroll
    for (int s = 0; s < 4 * NT; ++s) {
      const int n = 4 * s + lq;
      wf[s] = (k < a.K && n < a.N) ? a.W[(size_t)k * a.ldw + n] : 0.f;
    }
  }

  f32x4 accw[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) accw[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  // a row tile: x [16][64 k] one 16-byte piece per thread, dy [16][64 n] four values per thread; zeros beyond the
  // block's rows, K and N (they add nothing to dW and db; their dx is not stored)
  const int xr_row = tid >> 4, xr_k = 4 * (tid & 15);
  const bool xk_ok = kbase + xr_k < a.K;
  float4 xr[LN_SUPER];
  float dr[LN_SUPER][4];
#define LN_STORE(j_)                                                                                              \
  {                                                                                                               \
    *reinterpret_cast<float4 *>(&Xs[(j_) & 1][xr_row * LN_LDX + xr_k]) = xr[j_];                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
      const int idx = tid + 256 * i;                                                                              \
      Ds[(j_) & 1][(idx >> 6) * LN_LDD + (idx & 63)] = dr[j_][i];                                                 \
    }                                                                                                             \
  }

  for (int rs = r_begin; rs < r_end; rs += LN_SUPER * LN_ROWS) {
#pragma unroll
    for (int j = 0; j < LN_SUPER; ++j) {
      const int r = rs + LN_ROWS * j + xr_row;
      xr[j] = (r < r_end && xk_ok) ? *reinterpret_cast<const float4 *>(a.x + (size_t)r * a.ldx + kbase + xr_k)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < LN_SUPER; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, rr = rs + LN_ROWS * j + (idx >> 6), c = idx & 63;
        dr[j][i] = (rr < r_end && c < a.N) ? a.dy[(size_t)rr * a.ldy + c] : 0.f;
      }
    LN_STORE(0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LN_SUPER; ++j) {
      const int r0 = rs + LN_ROWS * j;
      if (r0 >= r_end) continue;                           // uniform over the workgroup (no break: the loop stays unrolled)
      // the next tile into the other buffer: its last readers passed the barrier that ended the previous tile
      if (j + 1 < LN_SUPER && r0 + LN_ROWS < r_end) LN_STORE(j + 1);
      const float *X = Xs[j & 1], *D = Ds[j & 1];

      if (a.dx) {
        // dx^T tile [16 k][16 rows] = W[16 k, N]·dy^T: two accumulators take the even and the odd steps (a dependent
        // MFMA waits 40 cycles, an independent one 32); the n order of a row's sum is the same for every row
        f32x4 e = f32x4{0.f, 0.f, 0.f, 0.f}, o = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *dp = &D[li * LN_LDD + lq];
#pragma unroll
        for (int s = 0; s < 4 * NT; s += 2) {
          e = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], dp[4 * s], e, 0, 0, 0);
          o = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s + 1], dp[4 * s + 4], o, 0, 0, 0);
        }
        const int r = r0 + li, k = kbase + 16 * w + 4 * lq;        // lane: row li, k = 4 lq + register
        if (r < r_end && k < a.K)
          *reinterpret_cast<float4 *>(a.dx + (size_t)r * a.lddx + k) =
              make_float4(e[0] + o[0], e[1] + o[1], e[2] + o[2], e[3] + o[3]);
      }
      // dW piece [16 k][N] += x_tile^T·dy_tile, the tile's rows in order
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float av = X[(4 * s + lq) * LN_LDX + 16 * w + li];
        const float *bp = &D[(4 * s + lq) * LN_LDD + li];
#pragma unroll
        for (int t = 0; t < NT; ++t) accw[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[16 * t], accw[t], 0, 0, 0);
      }
      if (blockIdx.x == 0 && tid < a.N) {
#pragma unroll
        for (int r = 0; r < LN_ROWS; ++r) dbacc += D[r * LN_LDD + tid];
      }
      __syncthreads();
    }
  }
#undef LN_STORE

  // lane: column n = 16 t + li, rows k = 4 lq + r of the wave's 16
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = 16 * t + li;
    if (n < a.N)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = kbase + 16 * w + 4 * lq + r;
        if (k < a.K) slab[(size_t)k * a.N + n] = accw[t][r];
      }
  }
  if (blockIdx.x == 0 && tid < a.N) slab[(size_t)a.K * a.N + tid] = dbacc;
}

// dW | db = the slabs added in block order (the loads of eight slabs in flight, the adds in order)
__global__ __launch_bounds__(256) void linear_narrow_reduce_kernel(const float *slab, int nblocks, int kn, int n,
                                                                   float *dW, float *db) {
  const int i = blockIdx.x * 256 + threadIdx.x, total = kn + n;
  if (i >= total) return;
  float s = 0.f;
  for (int b0 = 0; b0 < nblocks; b0 += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = b0 + j < nblocks ? slab[(size_t)(b0 + j) * total + i] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (b0 + j < nblocks) s += v[j];
  }
  if (i < kn) dW[i] = s;
  else db[i - kn] = s;
}

static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool linear_narrow_enabled() {
  static const int on = env_int("NABU_LINEAR_NARROW", 1);
  return on != 0;
}

bool linear_narrow_fwd_ok(int M, int N, int K, const float *A, int lda, const float *B, const float *C) {
  return linear_narrow_enabled() && M > 0 && N > 0 && N <= LN_MAXN && K > 0 && K % 4 == 0 && lda % 4 == 0 && al16(A) &&
         al16(B) && al16(C);
}

int linear_narrow_fwd(int M, int N, int K, float alpha, const float *A, int lda, const float *B, int ldb, float *C,
                      int ldc, const float *bias, hipStream_t s) {
  LinFwdArgs a;
  a.A = A; a.B = B; a.bias = bias; a.C = C;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
  a.alpha = alpha;
  a.vecB = N % 4 == 0 && ldb % 4 == 0;
  const dim3 grid((M + LN_ROWS - 1) / LN_ROWS), block(LN_FT);
  const size_t lds = (size_t)LN_KC * LN_LDB * sizeof(float);
  switch ((N + 15) / 16) {
    case 1: return launch_lds(linear_narrow_fwd_kernel<1>, grid, block, lds, s, a);
    case 2: return launch_lds(linear_narrow_fwd_kernel<2>, grid, block, lds, s, a);
    case 3: return launch_lds(linear_narrow_fwd_kernel<3>, grid, block, lds, s, a);
    default: return launch_lds(linear_narrow_fwd_kernel<4>, grid, block, lds, s, a);
  }
}

// rows of a backward row block: LN_TARGET_WGS workgroups over (k-slices x row blocks), whole row tiles
static int bwd_rows_per_block(int M, int K) {
  const int nks = (K + LN_KS - 1) / LN_KS;
  int nrb = (LN_TARGET_WGS + nks - 1) / nks;
  const int tiles = (M + LN_ROWS - 1) / LN_ROWS;
  if (nrb > tiles) nrb = tiles;
  if (nrb < 1) nrb = 1;
  return (tiles + nrb - 1) / nrb * LN_ROWS;
}

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_linear_bwd_ws_bytes(int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  const int rpb = bwd_rows_per_block(M, K), nrb = (M + rpb - 1) / rpb;
  return (size_t)nrb * ((size_t)K * N + N) * sizeof(float);
}

extern "C" int nabu_linear_bwd_f32(int M, int K, int N, const float *x, int ldx, const float *dy, int ldy,
                                   const float *W, int ldw, float *dx, int lddx, float *dW, float *db, void *ws,
                                   size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(M >= 0 && K >= 0 && N >= 0, "linear_bwd: negative dimension");
  NABU_CHECK_ARG(M > 0 && K > 0 && N > 0, "linear_bwd: empty dimension");
  NABU_CHECK_ARG(x && dy && W && dW && db, "linear_bwd: null pointer");
  NABU_CHECK_ARG(ldx >= K && ldy >= N && ldw >= N && (!dx || lddx >= K), "linear_bwd: leading dimension below the row length");
  if (!linear_narrow_enabled()) return fail(NABU_EUNSUP, "linear_bwd: switched off (NABU_LINEAR_NARROW=0)");
  if (N > LN_MAXN || K % 4 != 0 || ldx % 4 != 0 || (dx && lddx % 4 != 0) || !al16(x) || !al16(dy) || !al16(W) ||
      !al16(dx) || !al16(dW) || !al16(db))
    return fail(NABU_EUNSUP, "linear_bwd: needs N <= %d, K %% 4 == 0 and 16-byte aligned operands", LN_MAXN);
  const size_t need = nabu_linear_bwd_ws_bytes(M, K, N);
  if (!ws || ws_bytes < need) return fail(NABU_EWS, "linear_bwd: workspace %zu < %zu", ws_bytes, need);
  NABU_CHECK_ARG(al16(ws), "linear_bwd: workspace not 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  LinBwdArgs a;
  a.x = x; a.dy = dy; a.W = W; a.dx = dx; a.slab = static_cast<float *>(ws);
  a.M = M; a.K = K; a.N = N; a.ldx = ldx; a.ldy = ldy; a.ldw = ldw; a.lddx = lddx;
  a.rows_per_block = bwd_rows_per_block(M, K);
  const int nrb = (M + a.rows_per_block - 1) / a.rows_per_block, nks = (K + LN_KS - 1) / LN_KS;
  const dim3 grid(nks, nrb), block(256);
  switch ((N + 15) / 16) {
    case 1: NABU_TRY(launch_lds(linear_narrow_bwd_kernel<1>, grid, block, 0, s, a)); break;
    case 2: NABU_TRY(launch_lds(linear_narrow_bwd_kernel<2>, grid, block, 0, s, a)); break;
    case 3: NABU_TRY(launch_lds(linear_narrow_bwd_kernel<3>, grid, block, 0, s, a)); break;
    default: NABU_TRY(launch_lds(linear_narrow_bwd_kernel<4>, grid, block, 0, s, a)); break;
  }
  const int total = K * N + N;
  return launch_lds(linear_narrow_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, s,
                    static_cast<const float *>(ws), nrb, K * N, N, dW, db);
}
