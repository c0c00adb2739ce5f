// conv2d.hip — the convolutional front end of the BLSTM encoders: 3x3 "same" convolutions with bias and ReLU, their
// gradients and the 2x2 max-pool, on channels-last fp32 tensors x [B, T, F, C] with a length vector len [B].
//
// Forward (conv3x3_kernel) is an IMPLICIT GEMM on the exact-fp32 matrix instruction gemm.hip uses
// (v_mfma_f32_32x32x2_f32): M = a tile of (t, f) output positions of one utterance, N = Cout, K = 9 Cin.  No im2col
// matrix exists anywhere: a workgroup stages the input HALO tile — (CONV_TT + 2) frames x (tile_f + 2) bins x CONV_CK
// channels — in LDS once per channel chunk and reads all nine taps from it, so an input word is fetched once, not nine
// times.  LDS layout: one plane per channel, Xs[ci][frame][bin] with a constant row stride, so that the 32 lanes of an
// MFMA A operand (32 consecutive output positions) read 32 nearly consecutive words, and the offset of (tap, channel
// pair) is a compile-time immediate of the ds_read.  Weights of the chunk sit k-major, Ws[(tap, ci)][co], as gemm.hip
// lays out Bs.  Channels past Cin (Cin = 1 or 3: K = 9 or 27) are zero planes, and channel pairs past Cin are skipped.
// The next chunk's input and weights are fetched into registers under the current chunk's 72 MFMAs per wave.
// A wave owns 32 positions x 64 output channels; the four waves are arranged (rows x columns) as the tile needs:
// 4 x 1 for F = 41 (123 positions), 2 x 2 for F = 21 (63 positions), 1 x 2 below.
// The length rule (include/nabu_hip.h): frames >= len[b] read as zero and are written as zero.
// The data gradient is the same kernel on (dy . [y > 0]) and the flipped weights (MASK operand mode, plain epilogue).
//
// Weight gradient (conv3x3_wgrad_kernel): dw[tap] [Cin, Cout] = X_tap^T . G with the positions as the reduction, nine
// accumulator tiles (one per tap) per wave, all fed from the same halo tile; deterministic split-K over (b, time tile)
// into a workspace, summed in split order by a second launch together with the bias gradient.  No float atomics.
#include "gemm_args.h"

namespace nabu {

constexpr int CONV_TT = 3;                       // frames of an output tile (nabu_conv_tile_t)
constexpr int CONV_TF = 42;                      // widest tile in f: CONV_TT * CONV_TF <= 128 positions = 4 MFMA row blocks
constexpr int CONV_CK = 8;                       // channels per chunk: 72 reduction indices, 36 MFMA k-steps
constexpr int CONV_XROW = CONV_TF + 2;           // halo row stride (words)
constexpr int CONV_HP = (CONV_TT + 2) * CONV_XROW;   // halo positions: 220
constexpr int CONV_PLANE = CONV_HP + 8;          // channel plane stride
constexpr int CONV_GROW = CONV_TF;               // weight gradient: row stride of the position-major dy tile (even)

struct ConvArgs {
  const float *x, *mask, *w, *bias;
  float *y;
  const int32_t *len;
  int B, T, F, Cin, Cout;
  int nft, tf;      // tiles along f and their width
  int wr;           // waves along the positions (1, 2 or 4)
  int plain;        // no bias, no ReLU
};

static void conv_f_tiles(int F, int *nft, int *tf) {
  *nft = (F + CONV_TF - 1) / CONV_TF;
  *tf = (F + *nft - 1) / *nft;
}

// VEC: Cin % 4 == 0 and 16-byte aligned x (and mask): 16-byte loads of four channels; else word by word.
// MASK: the loaded input is multiplied by [mask > 0] (mask: a tensor of x's shape).  NW: output channels per workgroup.
template <bool VEC, bool MASK, int NW>
__global__ __launch_bounds__(256) void conv3x3_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  constexpr int LDW = NW + 4;
  constexpr int NXV = (CONV_HP * 2 + 255) / 256;               // 16-byte input pieces per thread (2)
  constexpr int NXS = (CONV_HP * CONV_CK + 255) / 256;         // input words per thread, scalar path (7)
  constexpr int NWV = (9 * CONV_CK * (NW / 4) + 255) / 256;    // 16-byte weight pieces per thread (5 or 9)
  float *Xs = csm, *Ws = csm + CONV_CK * CONV_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int b = blockIdx.z;
  const int t0 = (blockIdx.x / a.nft) * CONV_TT, f0 = (blockIdx.x % a.nft) * a.tf;
  const int tfw = min(a.tf, a.F - f0);
  const int n0 = blockIdx.y * NW;
  const int ncol = min(NW, a.Cout - n0);
  const int len = min(max(a.len[b], 0), a.T);
  const int rows = min(CONV_TT, a.T - t0);
  if (t0 >= len) {                                             // a tile of padding frames: zeros, nothing else
    for (int i = tid; i < rows * tfw * ncol; i += 256) {
      const int n = i % ncol, f = (i / ncol) % tfw, tt = i / (ncol * tfw);
      a.y[(((size_t)b * a.T + t0 + tt) * a.F + f0 + f) * a.Cout + n0 + n] = 0.f;
    }
    return;
  }
  const int npos = CONV_TT * tfw;
  const int WC = min(4 / a.wr, NW / 64), nw = a.wr * WC;       // waves past nw repeat another wave's work and store nothing
  const int wq = w % nw, wrow = wq % a.wr, wcol = wq / a.wr;
  const int mc = min(wrow * 32 + li, npos - 1);                // rows past the tile: a valid address, dropped at the store
  const float *a_ptr = Xs + lk * CONV_PLANE + (mc / tfw) * CONV_XROW + mc % tfw;
  const float *b_ptr = Ws + lk * LDW + wcol * 64 + li;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;

  float4 rxv[NXV];
  float rxs[NXS];
  float4 rw[NWV];
  auto gload = [&](int c0) {
    if (VEC) {
#pragma unroll
      for (int j = 0; j < NXV; ++j) {
        const int idx = tid + 256 * j, hp = idx >> 1, q = idx & 1;
        const int ht = hp / CONV_XROW, hf = hp % CONV_XROW;
        const int t = t0 - 1 + ht, f = f0 - 1 + hf, c = c0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hp < CONV_HP && hf < tfw + 2 && t >= 0 && t < len && f >= 0 && f < a.F && c < a.Cin) {
          const size_t off = (((size_t)b * a.T + t) * a.F + f) * a.Cin + c;
          v = *reinterpret_cast<const float4 *>(a.x + off);
          if (MASK) {
            const float4 m = *reinterpret_cast<const float4 *>(a.mask + off);
            v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
            v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
          }
        }
        rxv[j] = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < NXS; ++j) {
        const int idx = tid + 256 * j, hp = idx / CONV_CK, c = c0 + idx % CONV_CK;
        const int ht = hp / CONV_XROW, hf = hp % CONV_XROW;
        const int t = t0 - 1 + ht, f = f0 - 1 + hf;
        float v = 0.f;
        if (hp < CONV_HP && hf < tfw + 2 && t >= 0 && t < len && f >= 0 && f < a.F && c < a.Cin) {
          const size_t off = (((size_t)b * a.T + t) * a.F + f) * a.Cin + c;
          v = a.x[off];
          if (MASK) v = a.mask[off] > 0.f ? v : 0.f;
        }
        rxs[j] = v;
      }
    }
#pragma unroll
    for (int j = 0; j < NWV; ++j) {
      const int idx = tid + 256 * j, row = idx / (NW / 4), n = 4 * (idx % (NW / 4));
      const int tap = row / CONV_CK, c = c0 + row % CONV_CK;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < 9 * CONV_CK && c < a.Cin && n < ncol)          // (Cout % 32 == 0: a 16-byte piece is inside or outside)
        v = *reinterpret_cast<const float4 *>(a.w + ((size_t)tap * a.Cin + c) * a.Cout + n0 + n);
      rw[j] = v;
    }
  };
  auto sstore = [&]() {
    if (VEC) {
#pragma unroll
      for (int j = 0; j < NXV; ++j) {
        const int idx = tid + 256 * j, hp = idx >> 1, q = idx & 1;
        if (hp < CONV_HP) {
          float *d = Xs + 4 * q * CONV_PLANE + hp;
          d[0] = rxv[j].x; d[CONV_PLANE] = rxv[j].y; d[2 * CONV_PLANE] = rxv[j].z; d[3 * CONV_PLANE] = rxv[j].w;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NXS; ++j) {
        const int idx = tid + 256 * j, hp = idx / CONV_CK;
        if (hp < CONV_HP) Xs[(idx % CONV_CK) * CONV_PLANE + hp] = rxs[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NWV; ++j) {
      const int idx = tid + 256 * j, row = idx / (NW / 4), n = 4 * (idx % (NW / 4));
      if (row < 9 * CONV_CK) *reinterpret_cast<float4 *>(Ws + row * LDW + n) = rw[j];
    }
  };

  gload(0);
  sstore();
  __syncthreads();
  for (int c0 = 0; c0 < a.Cin; c0 += CONV_CK) {
    const bool more = c0 + CONV_CK < a.Cin;
    if (more) gload(c0 + CONV_CK);
    const int kpairs = (min(CONV_CK, a.Cin - c0) + 1) >> 1;    // an odd channel count: its partner is a zero plane
#define NABU_CONV_KSTEP(tap, kp)                                                              \
  {                                                                                         \
    const float av = a_ptr[((tap) / 3) * CONV_XROW + (tap) % 3 + 2 * (kp) * CONV_PLANE];    \
    const float b0 = b_ptr[((tap) * CONV_CK + 2 * (kp)) * LDW];                             \
    const float b1 = b_ptr[((tap) * CONV_CK + 2 * (kp)) * LDW + 32];                        \
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc0, 0, 0, 0);                     \
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc1, 0, 0, 0);                     \
  }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kp = 0; kp < CONV_CK / 2; ++kp)
        if (kp < kpairs) NABU_CONV_KSTEP(tap, kp)
#undef NABU_CONV_KSTEP
    __syncthreads();
    if (more) {
      sstore();
      __syncthreads();
    }
  }

  // epilogue: a lane holds column (lane & 31), rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of its 32 x 32 tiles
  if (w >= nw) return;
  const int rbase = 4 * lk;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int nl = wcol * 64 + ni * 32 + li;
    if (nl >= ncol) continue;
    const float bv = a.plain ? 0.f : a.bias[n0 + nl];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = wrow * 32 + (r & 3) + 8 * (r >> 2) + rbase;
      if (m >= npos) continue;
      const int tt = m / tfw, f = m % tfw;
      if (tt >= rows) continue;
      const float s = ni ? acc1[r] : acc0[r];
      float v = a.plain ? s : relu_value(s + bv);
      if (t0 + tt >= len) v = 0.f;
      a.y[(((size_t)b * a.T + t0 + tt) * a.F + f0 + f) * a.Cout + n0 + nl] = v;
    }
  }
}

// w'[kt, kf, co, ci] = w[2 - kt, 2 - kf, ci, co]: the weights of the data-gradient convolution
__global__ __launch_bounds__(256) void conv3x3_flip_kernel(int Cin, int Cout, const float *w, float *wf) {
  const int total = 9 * Cin * Cout;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int ci = i % Cin, co = (i / Cin) % Cout, tap = i / (Cin * Cout);
    wf[i] = w[((size_t)(8 - tap) * Cin + ci) * Cout + co];
  }
}

struct WgradArgs {
  const float *x, *dy, *y;
  float *part;      // [nsplit][9 Cin Cout] then [nsplit][Cout]
  const int32_t *len;
  int B, T, F, Cin, Cout;
  int nft, tf, ntt;         // tiles along f, their width, tiles along t
  int per, nsplit;          // (b, time tile) pairs per split
};

// CIB x COB waves: a wave owns 32 input channels x 32 output channels of all nine taps (nine accumulator tiles)
template <int CIB, int COB>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float csm[];
  constexpr int NCI = CIB * 32, NCO = COB * 32, LDX = NCI + 1, LDG = NCO + 4;
  constexpr int GROWS = CONV_TT * CONV_GROW;
  float *Xs = csm;                                            // [halo position][channel], odd stride
  float *Gs = csm + ((CONV_HP * LDX + 3) & ~3);               // [position][output channel]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int wi = w % CIB, wo = w / CIB;
  const int c0 = blockIdx.x * NCI, n0 = blockIdx.y * NCO, z = blockIdx.z;
  const int nci = min(NCI, a.Cin - c0), nco = min(NCO, a.Cout - n0);
  const bool vecx = a.Cin % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int total = a.B * a.ntt;
  const int first = z * a.per, last = min(first + a.per, total);
  for (int tile = first; tile < last; ++tile) {
    const int b = tile / a.ntt, t0 = (tile % a.ntt) * CONV_TT;
    const int len = min(max(a.len[b], 0), a.T);
    if (t0 >= len) continue;                                  // padding frames add nothing (uniform in the workgroup)
    for (int ft = 0; ft < a.nft; ++ft) {
      const int f0 = ft * a.tf, tfw = min(a.tf, a.F - f0);
      __syncthreads();                                        // the previous tile has been read
      if (vecx) {
        for (int idx = tid; idx < CONV_HP * (NCI / 4); idx += 256) {
          const int hp = idx / (NCI / 4), c = 4 * (idx % (NCI / 4));
          const int hf = hp % CONV_XROW, t = t0 - 1 + hp / CONV_XROW, f = f0 - 1 + hf;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (hf < tfw + 2 && t >= 0 && t < len && f >= 0 && f < a.F && c < nci)     // (past the halo: zero, as in the forward kernel)
            v = *reinterpret_cast<const float4 *>(a.x + (((size_t)b * a.T + t) * a.F + f) * a.Cin + c0 + c);
          float *d = Xs + hp * LDX + c;
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
      } else {
        for (int idx = tid; idx < CONV_HP * NCI; idx += 256) {
          const int hp = idx / NCI, c = idx % NCI;
          const int hf = hp % CONV_XROW, t = t0 - 1 + hp / CONV_XROW, f = f0 - 1 + hf;
          float v = 0.f;
          if (hf < tfw + 2 && t >= 0 && t < len && f >= 0 && f < a.F && c < nci)
            v = a.x[(((size_t)b * a.T + t) * a.F + f) * a.Cin + c0 + c];
          Xs[hp * LDX + c] = v;
        }
      }
      for (int idx = tid; idx < GROWS * (NCO / 4); idx += 256) {
        const int row = idx / (NCO / 4), n = 4 * (idx % (NCO / 4));
        const int t = t0 + row / CONV_GROW, f = row % CONV_GROW;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < len && f < tfw && n < nco) {
          const size_t off = (((size_t)b * a.T + t) * a.F + f0 + f) * a.Cout + n0 + n;
          v = *reinterpret_cast<const float4 *>(a.dy + off);
          const float4 m = *reinterpret_cast<const float4 *>(a.y + off);
          v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f;
          v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
        }
        *reinterpret_cast<float4 *>(Gs + row * LDG + n) = v;
      }
      __syncthreads();
      const float *xp = Xs + lk * LDX + wi * 32 + li;
      const float *gp = Gs + lk * LDG + wo * 32 + li;
#pragma unroll
      for (int tt = 0; tt < CONV_TT; ++tt)
        for (int f = 0; f < tfw; f += 2) {                    // positions (tt, f + lk); f + 1 == tfw is a zero row of Gs
          const float g = gp[(tt * CONV_GROW + f) * LDG];
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            const float xv = xp[((tt + tap / 3) * CONV_XROW + f + tap % 3) * LDX];
            acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, g, acc[tap], 0, 0, 0);
          }
        }
      if (blockIdx.x == 0 && tid < NCO)                       // bias gradient: the columns of the same tile, in row order
        for (int row = 0; row < GROWS; ++row) bsum += Gs[row * LDG + tid];
    }
  }
  const size_t wsz = (size_t)9 * a.Cin * a.Cout;
  float *part = a.part + (size_t)z * wsz;
  const int co = wo * 32 + li;
  if (co < nco) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (ci < nci) part[((size_t)tap * a.Cin + c0 + ci) * a.Cout + n0 + co] = acc[tap][r];
      }
  }
  if (blockIdx.x == 0 && tid < nco) a.part[(size_t)a.nsplit * wsz + (size_t)z * a.Cout + n0 + tid] = bsum;
}

__global__ __launch_bounds__(256) void conv3x3_wgrad_sum_kernel(int nsplit, size_t wsz, int Cout, const float *part,
                                                                 float *dw, float *dbias) {
  const size_t total = wsz + Cout;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const bool isw = i < wsz;
    const float *p = isw ? part + i : part + (size_t)nsplit * wsz + (i - wsz);
    const size_t stride = isw ? wsz : (size_t)Cout;
    float s = 0.f;
    for (int z = 0; z < nsplit; ++z) s += p[(size_t)z * stride];
    if (isw) dw[i] = s; else dbias[i - wsz] = s;
  }
}

static void wgrad_shape(int Cin, int Cout, int *cib, int *cob) {
  // (Cin <= 32 has one block of input channels: the four waves go along Cout, and those past it idle)
  *cob = (Cout >= 128 || Cin <= 32) ? 4 : Cout >= 64 ? 2 : 1;
  *cib = 4 / *cob;
}
static int wgrad_splits(int B, int T, int Cin, int Cout, int *per) {
  int cib, cob;
  wgrad_shape(Cin, Cout, &cib, &cob);
  const int groups = ((Cin + cib * 32 - 1) / (cib * 32)) * ((Cout + cob * 32 - 1) / (cob * 32));
  const int total = B * ((T + CONV_TT - 1) / CONV_TT);
  int ns = (512 + groups - 1) / groups;                       // two workgroups per CU of a whole chip
  const int most = (total + 3) / 4;                           // at least four (b, time tile) pairs per split
  if (ns > most) ns = most;
  if (ns < 1) ns = 1;
  *per = (total + ns - 1) / ns;
  return (total + *per - 1) / *per;
}

// 2x2 max-pool, ceil mode: a window takes frames < len[b] and bins < F only
__global__ __launch_bounds__(256) void maxpool2x2_fwd_kernel(int B, int T, int F, int C, const float *x,
                                                              const int32_t *len, float *y) {
  const int Tp = (T + 1) / 2, Fp = (F + 1) / 2;
  const size_t total = (size_t)B * Tp * Fp * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C), fp = (int)(i / C % Fp), tp = (int)(i / ((size_t)C * Fp) % Tp);
    const int b = (int)(i / ((size_t)C * Fp * Tp));
    const int l = min(max(len[b], 0), T);
    float v = 0.f;
    if (2 * tp < l) {
      const float *p = x + (((size_t)b * T + 2 * tp) * F + 2 * fp) * C + c;
      v = p[0];
      if (2 * fp + 1 < F) v = fmaxf(v, p[C]);
      if (2 * tp + 1 < l) {
        v = fmaxf(v, p[(size_t)F * C]);
        if (2 * fp + 1 < F) v = fmaxf(v, p[(size_t)F * C + C]);
      }
    }
    y[i] = v;
  }
}
// the gradient goes to the FIRST maximum of the window in (t, f) order
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(int B, int T, int F, int C, const float *x,
                                                              const int32_t *len, const float *dy, float *dx) {
  const int Tp = (T + 1) / 2, Fp = (F + 1) / 2;
  const size_t total = (size_t)B * T * F * C;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C), f = (int)(i / C % F), t = (int)(i / ((size_t)C * F) % T);
    const int b = (int)(i / ((size_t)C * F * T));
    const int l = min(max(len[b], 0), T);
    float v = 0.f;
    if (t < l) {
      const int tp = t >> 1, fp = f >> 1;
      const float *p = x + (((size_t)b * T + 2 * tp) * F + 2 * fp) * C + c;
      float best = p[0];
      int arg = 0;
      if (2 * fp + 1 < F && p[C] > best) { best = p[C]; arg = 1; }
      if (2 * tp + 1 < l) {
        if (p[(size_t)F * C] > best) { best = p[(size_t)F * C]; arg = 2; }
        if (2 * fp + 1 < F && p[(size_t)F * C + C] > best) arg = 3;
      }
      if (arg == 2 * (t & 1) + (f & 1)) v = dy[(((size_t)b * Tp + tp) * Fp + fp) * C + c];
    }
    dx[i] = v;
  }
}

// y[n, f, c] = x[n, c F + f]: the equal column blocks of a feature vector (static, delta, delta-delta) as channels
__global__ __launch_bounds__(256) void blocks_to_channels_kernel(size_t N, int C, int F, const float *x, float *y) {
  const size_t total = N * C * F;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % C), f = (int)(i / C % F);
    y[i] = x[(i / ((size_t)C * F)) * C * F + (size_t)c * F + f];
  }
}

static unsigned pool_blocks(size_t total) { return (unsigned)min((total + 255) / 256, (size_t)8192); }
static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool VEC, bool MASK>
static int conv_launch(const ConvArgs &a, int nw, dim3 grid, hipStream_t s) {
  const size_t lds = ((size_t)CONV_CK * CONV_PLANE + (size_t)9 * CONV_CK * (nw + 4)) * sizeof(float);
  return nw == 128 ? launch_lds(conv3x3_kernel<VEC, MASK, 128>, grid, dim3(256), lds, s, a)
                   : launch_lds(conv3x3_kernel<VEC, MASK, 64>, grid, dim3(256), lds, s, a);
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_conv_tile_t(void) { return CONV_TT; }

extern "C" int nabu_blocks_to_channels_f32(size_t N, int C, int F, const float *x, float *y, nabu_stream_t stream) {
  NABU_CHECK_ARG(C >= 1 && F >= 1, "blocks_to_channels: bad dimensions");
  NABU_CHECK_ARG(x && y, "blocks_to_channels: null pointer");
  if (N == 0) return 0;
  hipLaunchKernelGGL(blocks_to_channels_kernel, dim3(pool_blocks(N * C * F)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     N, C, F, x, y);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_conv3x3_relu_fwd(int B, int T, int F, int Cin, int Cout, const float *x, const float *mask,
                                     const int32_t *len, const float *w, const float *bias, int plain, float *y,
                                     nabu_stream_t stream) {
  NABU_CHECK_ARG(B >= 0 && T >= 0, "conv3x3: negative batch or time dimension");
  NABU_CHECK_ARG(F >= 1, "conv3x3: F = %d, must be >= 1", F);
  NABU_CHECK_ARG(Cin >= 1, "conv3x3: Cin = %d, must be >= 1", Cin);
  NABU_CHECK_ARG(Cout >= 32 && Cout % 32 == 0, "conv3x3: Cout = %d is not a positive multiple of 32", Cout);
  NABU_CHECK_ARG(B <= 65535, "conv3x3: B = %d > 65535", B);
  NABU_CHECK_ARG(x && len && w && y && (plain || bias), "conv3x3: null pointer");
  NABU_CHECK_ARG(al16(w), "conv3x3: the weights must be 16-byte aligned");
  if (B == 0 || T == 0) return 0;
  ConvArgs a;
  a.x = x; a.mask = mask; a.w = w; a.bias = bias; a.y = y; a.len = len;
  a.B = B; a.T = T; a.F = F; a.Cin = Cin; a.Cout = Cout; a.plain = plain;
  conv_f_tiles(F, &a.nft, &a.tf);
  const int nrb = (CONV_TT * a.tf + 31) / 32;
  a.wr = nrb > 2 ? 4 : nrb;
  const int nw = (Cout >= 128 && a.wr <= 2) ? 128 : 64;
  const dim3 grid(((T + CONV_TT - 1) / CONV_TT) * a.nft, (Cout + nw - 1) / nw, B);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = Cin % 4 == 0 && al16(x) && (!mask || al16(mask));
  if (mask) return vec ? conv_launch<true, true>(a, nw, grid, s) : conv_launch<false, true>(a, nw, grid, s);
  return vec ? conv_launch<true, false>(a, nw, grid, s) : conv_launch<false, false>(a, nw, grid, s);
}

extern "C" int nabu_conv3x3_flip_weights(int Cin, int Cout, const float *w, float *w_flipped, nabu_stream_t stream) {
  NABU_CHECK_ARG(Cin >= 1 && Cout >= 1, "conv3x3_flip_weights: bad dimensions");
  NABU_CHECK_ARG(w && w_flipped, "conv3x3_flip_weights: null pointer");
  const int total = 9 * Cin * Cout;
  hipLaunchKernelGGL(conv3x3_flip_kernel, dim3(min((total + 255) / 256, 1024)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), Cin, Cout, w, w_flipped);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t nabu_conv_ws_bytes(int B, int T, int F, int Cin, int Cout) {
  if (B <= 0 || T <= 0 || F < 1 || Cin < 1 || Cout < 32 || Cout % 32) return 0;
  int per;
  const int ns = wgrad_splits(B, T, Cin, Cout, &per);
  return (size_t)ns * ((size_t)9 * Cin * Cout + Cout) * sizeof(float);
}

extern "C" int nabu_conv3x3_bwd_weights(int B, int T, int F, int Cin, int Cout, const float *x, const float *dy,
                                        const float *y, const int32_t *len, float *dw, float *dbias, void *ws,
                                        size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(B >= 1 && T >= 1, "conv3x3_bwd_weights: empty batch");
  NABU_CHECK_ARG(F >= 1, "conv3x3_bwd_weights: F = %d, must be >= 1", F);
  NABU_CHECK_ARG(Cin >= 1, "conv3x3_bwd_weights: Cin = %d, must be >= 1", Cin);
  NABU_CHECK_ARG(Cout >= 32 && Cout % 32 == 0, "conv3x3_bwd_weights: Cout = %d is not a positive multiple of 32", Cout);
  NABU_CHECK_ARG(x && dy && y && len && dw && dbias && ws, "conv3x3_bwd_weights: null pointer");
  NABU_CHECK_ARG(al16(dy) && al16(y) && al16(ws), "conv3x3_bwd_weights: dy, y and ws must be 16-byte aligned");
  if (ws_bytes < nabu_conv_ws_bytes(B, T, F, Cin, Cout)) return fail(NABU_EWS, "conv3x3_bwd_weights: workspace too small");
  WgradArgs a;
  a.x = x; a.dy = dy; a.y = y; a.part = static_cast<float *>(ws); a.len = len;
  a.B = B; a.T = T; a.F = F; a.Cin = Cin; a.Cout = Cout;
  conv_f_tiles(F, &a.nft, &a.tf);
  a.ntt = (T + CONV_TT - 1) / CONV_TT;
  a.nsplit = wgrad_splits(B, T, Cin, Cout, &a.per);
  int cib, cob;
  wgrad_shape(Cin, Cout, &cib, &cob);
  const dim3 grid((Cin + cib * 32 - 1) / (cib * 32), (Cout + cob * 32 - 1) / (cob * 32), a.nsplit);
  const size_t lds = ((size_t)((CONV_HP * (cib * 32 + 1) + 3) & ~3) + (size_t)CONV_TT * CONV_GROW * (cob * 32 + 4)) * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  NABU_TRY(cob == 4   ? launch_lds(conv3x3_wgrad_kernel<1, 4>, grid, dim3(256), lds, s, a)
           : cob == 2 ? launch_lds(conv3x3_wgrad_kernel<2, 2>, grid, dim3(256), lds, s, a)
                      : launch_lds(conv3x3_wgrad_kernel<4, 1>, grid, dim3(256), lds, s, a));
  const size_t wsz = (size_t)9 * Cin * Cout;
  hipLaunchKernelGGL(conv3x3_wgrad_sum_kernel, dim3((unsigned)min((wsz + Cout + 255) / 256, (size_t)2048)), dim3(256), 0, s,
                     a.nsplit, wsz, Cout, a.part, dw, dbias);
  NABU_LAUNCH_CHECK();
  return 0;
}

static int pool_args(const char *what, int B, int T, int F, int C, const void *p0, const void *p1, const void *p2,
                     const void *p3) {
  NABU_CHECK_ARG(B >= 0 && T >= 0 && C >= 1, "%s: bad dimensions", what);
  NABU_CHECK_ARG(F >= 1, "%s: F = %d, must be >= 1", what, F);
  NABU_CHECK_ARG(p0 && p1 && p2 && p3, "%s: null pointer", what);
  return 0;
}

extern "C" int nabu_maxpool2x2_fwd(int B, int T, int F, int C, const float *x, const int32_t *len, float *y,
                                   nabu_stream_t stream) {
  NABU_TRY(pool_args("maxpool2x2_fwd", B, T, F, C, x, len, y, y));
  const size_t total = (size_t)B * ((T + 1) / 2) * ((F + 1) / 2) * C;
  if (total == 0) return 0;
  hipLaunchKernelGGL(maxpool2x2_fwd_kernel, dim3(pool_blocks(total)), dim3(256), 0, static_cast<hipStream_t>(stream), B, T,
                     F, C, x, len, y);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_maxpool2x2_bwd(int B, int T, int F, int C, const float *x, const int32_t *len, const float *dy,
                                   float *dx, nabu_stream_t stream) {
  NABU_TRY(pool_args("maxpool2x2_bwd", B, T, F, C, x, len, dy, dx));
  const size_t total = (size_t)B * T * F * C;
  if (total == 0) return 0;
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(pool_blocks(total)), dim3(256), 0, static_cast<hipStream_t>(stream), B, T,
                     F, C, x, len, dy, dx);
  NABU_LAUNCH_CHECK();
  return 0;
}
