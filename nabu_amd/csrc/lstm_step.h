// lstm_step.h — the launch-per-step (stepwise) recurrence of a BLSTM layer, shared by its two cells:
//   * the tiling of the recurrent products and the two product tiles themselves.  The plain cell (lstm.hip) fuses its
//     gate arithmetic behind a tile in the same launch; the layer-normalised cell (lstm_ln.hip) needs all H units of a
//     row for its statistics and runs them as a second launch.  Where the h state lives is the caller's business: the
//     tiles take the pointer.  Everything else they read from the kernel's argument struct (StepArgs of lstm.hip,
//     LnArgs below: B, T, D, H, len, kernel[2], gates[2]) where they need it — handing the kernel pointer in as a value
//     makes the compiler fetch it in the prologue, a second dependent kernel-argument fetch in front of the staging
//     loads, and costs every launch 0.3 us (LABNOTES.md, section 15).
//   * what lstm.hip's layer driver needs of the layer-normalised recurrence (lstm_ln.hip).
#pragma once
#include "common.h"

namespace nabu {

constexpr int SB = 16;    // batch rows per workgroup of the recurrent products
constexpr int SU = 16;    // hidden units per workgroup of the recurrent products
constexpr int DZC = 512;  // dz columns staged per LDS chunk (backward product)
constexpr int STEP_NT = 256;   // threads of every stepwise kernel (4 waves); grid of the products (H/SU, B/SB, 2)

// forward: zs[bl][g][u] = sum_k h_{s-1}[b0 + bl][k] · Wh[k][g H + u0 + u].  hprev [B][H] of this direction; Wh = rows
// [D, D + H) of p.kernel[dir]; LDS: hs [SB][H] (the staged rows: still valid on return), zs [SB][4][SU].  Ends with a
// barrier: every thread may read all of zs.
template <class Args>
__device__ __forceinline__ void rec_fwd_tile(const Args &p, const float *hprev, int dir, int b0, int u0, float *hs, float *zs) {
  const int H = p.H, B = p.B;
  const int tid = threadIdx.x;
  // stage h_{s-1} of this block's batch rows
  for (int i = tid; i < SB * H / 4; i += STEP_NT) {
    const int bl = i / (H / 4), k4 = i % (H / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 + bl < B) v = reinterpret_cast<const float4 *>(hprev + (size_t)(b0 + bl) * H)[k4];
    reinterpret_cast<float4 *>(hs + bl * H)[k4] = v;
  }
  __syncthreads();
  {  // thread = (batch row bl, gate g, unit quad q)
    const int q = tid & 3, g = (tid >> 2) & 3, bl = tid >> 4;
    const int ucol = u0 + 4 * q;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ucol < H) {
      const float *W = p.kernel[dir] + (size_t)p.D * 4 * H + (size_t)g * H + ucol;
      const float *hrow = hs + bl * H;
#pragma unroll 4
      for (int k = 0; k < H; ++k) {
        const float4 w = *reinterpret_cast<const float4 *>(W + (size_t)k * 4 * H);
        const float hv = hrow[k];
        acc.x = fmaf(hv, w.x, acc.x);
        acc.y = fmaf(hv, w.y, acc.y);
        acc.z = fmaf(hv, w.z, acc.z);
        acc.w = fmaf(hv, w.w, acc.w);
      }
    }
    *reinterpret_cast<float4 *>(zs + (bl * 4 + g) * SU + 4 * q) = acc;
  }
  __syncthreads();
}

// backward: returns dh[b0 + bl][u0 + u] = sum_col dz_{s+1}[b][col] · Wh[u][col] for thread (bl = tid / 16, u = tid % 16);
// 0 where that element lies outside B x H.  dz = p.gates[dir] [B][T][4H] (rows of finished sequences count as 0),
// staged through dzs in chunks of DZC columns.
template <class Args>
__device__ __forceinline__ float rec_bwd_tile(const Args &p, int dir, int s, int b0, int u0, float (*dzs)[DZC]) {
  const int H = p.H, B = p.B, T = p.T;
  const int tid = threadIdx.x;
  const int u = tid & 15, bl = tid >> 4;
  const int hu = u0 + u;
  const bool valid = b0 + bl < B && hu < H;
  float dh = 0.f;
  const float *Wrow = p.kernel[dir] + (size_t)(p.D + (hu < H ? hu : 0)) * 4 * H;
  for (int c0 = 0; c0 < 4 * H; c0 += DZC) {
    const int cw = min(DZC, 4 * H - c0);
    __syncthreads();
    for (int i = tid; i < SB * (DZC / 4); i += STEP_NT) {
      const int r = i / (DZC / 4), c4 = i % (DZC / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int bb = b0 + r;
      if (bb < B && 4 * c4 < cw) {
        const int nn = p.len[bb];
        if (s + 1 < nn) {
          const int t1 = dir ? nn - 2 - s : s + 1;
          v = *reinterpret_cast<const float4 *>(p.gates[dir] + ((size_t)bb * T + t1) * 4 * H + c0 + 4 * c4);
        }
      }
      *reinterpret_cast<float4 *>(&dzs[r][4 * c4]) = v;
    }
    __syncthreads();
    if (valid) {
#pragma unroll 4
      for (int c = 0; c < cw; c += 4) {
        const float4 w = *reinterpret_cast<const float4 *>(Wrow + c0 + c);
        const float4 d = *reinterpret_cast<const float4 *>(&dzs[bl][c]);
        dh = fmaf(d.x, w.x, dh);
        dh = fmaf(d.y, w.y, dh);
        dh = fmaf(d.z, w.z, dh);
        dh = fmaf(d.w, w.w, dh);
      }
    }
  }
  return dh;
}

// ---------------------------------------------------------------------------
// the layer-normalised recurrence (lstm_ln.hip), as lstm.hip's driver sees it
struct LnArgs {
  int B, T, D, H, max_len, save, has_dh;
  const int32_t *len;
  const float *kernel[2];
  float *gates[2], *cs[2], *rstd[2], *rstdc[2];   // (the reserve: lstm_ln.hip's header)
  const float *gamma[2][5], *beta[2][5];
  float *out;
  const float *dout;
  float *hstate;   // [2 dir][B][H]
  float *cstate;   // forward: the carried (normalised) c; backward: the dc carry.  [2][B][H]
  float *dh;       // backward: dz_{s+1} · Wh^T  [2][B][H]
  float *part;     // backward: per-row sums of the norm-parameter gradients [2][B][10][H] (0..4 dgamma, 5..9 dbeta)
};
size_t ln_lds_bytes(int H);      // the most LDS a workgroup of that family takes
// the steps of one pass over zeroed states: two launches each (the first step of a pass has no recurrent product)
int ln_recurrence_fwd(LnArgs p, hipStream_t s);
int ln_recurrence_bwd(LnArgs p, hipStream_t s);
// dgamma / dbeta from p.part (zeroed before ln_recurrence_bwd): one launch behind the recurrence
int ln_param_grads(const LnArgs &p, const nabu_blstm_ln_params *ln, hipStream_t s);

}  // namespace nabu
