// lstm_ln.hip — one bidirectional LSTM layer with layer normalisation inside the cell (layer.blstm(layer_norm=True),
// tf.contrib.rnn.LayerNormBasicLSTMCell(layer_norm=True); the semantics are stated in include/nabu_hip.h).
//
// The exact-fp32, launch-per-step family of lstm.hip: the row statistics of a step need all H units of a row, so a step
// is TWO launches, both directions in each:
//   forward   ln_rec_fwd_kernel   z[b,t] += h_{s-1} · Wh            grid (H/16, B/16, 2)  (lstm.hip's tiling)
//             ln_cell_fwd_kernel  statistics, gates, state norm, h   grid (B, 2): one workgroup per row and direction
//   backward  ln_rec_bwd_kernel   dh = dz_{s+1} · Wh^T              grid (H/16, B/16, 2)
//             ln_cell_bwd_kernel  cell and norm gradients, dz        grid (B, 2)
// Row statistics: two-pass (mean, then the centred squares) sums of 256 threads — a butterfly inside each wave, the four
// wave sums added in one fixed order.  The gamma/beta gradients are running sums per (direction, row) in the workspace,
// each owned by the one workgroup of that row, and are added over the rows in ascending order by one launch behind the
// recurrence: no floating-point atomics anywhere.
//
// reserve (fp32, batch-major):
//   zh_fw | zh_bw [B,T,4H]   x·Wx (GEMM output), then z (ln_rec_fwd), then the normalised z_hat (ln_cell_fwd), then dz —
//                            the gradient w.r.t. the pre-normalisation z (ln_cell_bwd); all in place
//   ch_fw | ch_bw [B,T,H]    the normalised new cell state before gamma/beta (stands where lstm.hip keeps cs)
//   rstd_fw | rstd_bw [B,T,4], rstdc_fw | rstdc_bw [B,T]
// A forward-only call uses zh alone and writes nothing back into it behind z.
#include "common.h"

#include <string.h>
#include <mutex>

namespace nabu {
namespace {

constexpr float LN_EPS = 1e-12f;
constexpr int SB = 16;    // batch rows per workgroup of the recurrent products
constexpr int SU = 16;    // hidden units per workgroup of the recurrent products
constexpr int DZC = 512;  // dz columns staged per LDS chunk (backward product)
constexpr int NT = 256;   // threads of every kernel here (4 waves)

struct LnArgs {
  int B, T, D, H, max_len, save, has_dh;
  const int32_t *len;
  const float *kernel[2];
  float *zh[2], *ch[2], *rstd[2], *rstdc[2];
  const float *gamma[2][5], *beta[2][5];
  float *out;
  const float *dout;
  float *hstate;   // [2 dir][B][H]
  float *cstate;   // forward: the carried (normalised) c; backward: the dc carry.  [2][B][H]
  float *dh;       // backward: dz_{s+1} · Wh^T  [2][B][H]
  float *part;     // backward: per-row sums of the norm-parameter gradients [2][B][10][H] (0..4 dgamma, 5..9 dbeta)
};

// sums of N values over the 256 threads of the workgroup, the same bits in every thread: xor butterfly inside a wave
// (both partners add the same two numbers), then the four wave sums as (w0 + w1) + (w2 + w3).  red: 4 * N floats of LDS.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float *red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] += __shfl_xor(v[n], off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();     // the previous sum's readers are done with red
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[wave * N + n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = (red[n] + red[N + n]) + (red[2 * N + n] + red[3 * N + n]);
}

// ---------------------------------------------------------------------------
// forward, launch 1 of a step: z[b,t] += h_{s-1}[b] · Wh for the rows still running (lstm_step_fwd_kernel's tiling)
__global__ __launch_bounds__(NT) void ln_rec_fwd_kernel(LnArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, B = p.B, T = p.T;
  float *hs = smem;               // [SB][H]
  float *zs = smem + SB * H;      // [SB][4][SU]
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int tid = threadIdx.x;
  const float *hprev = p.hstate + (size_t)dir * B * H;

  for (int i = tid; i < SB * H / 4; i += NT) {
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
  {  // thread = (batch row bl, unit u)
    const int u = tid & 15, bl = tid >> 4;
    const int b = b0 + bl, hu = u0 + u;
    if (b < B && hu < H) {
      const int n = p.len[b];
      if (s < n) {
        const int t = dir ? n - 1 - s : s;
        float *gp = p.zh[dir] + ((size_t)b * T + t) * 4 * H + hu;
#pragma unroll
        for (int k = 0; k < 4; ++k) gp[(size_t)k * H] += zs[(bl * 4 + k) * SU + u];
      }
    }
  }
}

// forward, launch 2 of a step: one workgroup per (row b, direction).  LDS: zs [4H] | cr [H] | red [16]
__global__ __launch_bounds__(NT) void ln_cell_fwd_kernel(LnArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, T = p.T;
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int n = p.len[b];
  if (s >= n) {   // finished sequence: state frozen, output row s is zero (t >= len)
    float *o = p.out + ((size_t)b * T + s) * 2 * H + (size_t)dir * H;
    for (int i = tid; i < H; i += NT) o[i] = 0.f;
    return;
  }
  float *zs = smem, *cr = smem + 4 * H, *red = smem + 5 * H;
  const int t = dir ? n - 1 - s : s;
  const size_t row = (size_t)b * T + t;
  float *gp = p.zh[dir] + row * 4 * H;
  const float invH = 1.0f / (float)H;

  float mean[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < H; i += NT)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = gp[k * H + i];
      zs[k * H + i] = v;          // (every thread reads back only what it wrote: no barrier)
      mean[k] += v;
    }
  block_sum<4>(mean, red);
  float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) mean[k] *= invH;
  for (int i = tid; i < H; i += NT)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = zs[k * H + i] - mean[k];
      rs[k] = fmaf(d, d, rs[k]);
    }
  block_sum<4>(rs, red);
#pragma unroll
  for (int k = 0; k < 4; ++k) rs[k] = 1.0f / sqrtf(rs[k] * invH + LN_EPS);

  float *cst = p.cstate + ((size_t)dir * p.B + b) * H;
  float mc[1] = {0.f};
  for (int i = tid; i < H; i += NT) {
    float a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = (zs[k * H + i] - mean[k]) * rs[k];
      if (p.save) gp[k * H + i] = xh;
      a[k] = fmaf(p.gamma[dir][k][i], xh, p.beta[dir][k][i]);
    }
    const float ig = sigmoidf_(a[0]), g = tanhf_(a[1]), f = sigmoidf_(a[2] + 1.0f), o = sigmoidf_(a[3]);
    const float c = cst[i] * f + ig * g;
    cr[i] = c;
    zs[3 * H + i] = o;
    mc[0] += c;
  }
  block_sum<1>(mc, red);
  const float meanc = mc[0] * invH;
  float vc[1] = {0.f};
  for (int i = tid; i < H; i += NT) {
    const float d = cr[i] - meanc;
    vc[0] = fmaf(d, d, vc[0]);
  }
  block_sum<1>(vc, red);
  const float rc = 1.0f / sqrtf(vc[0] * invH + LN_EPS);

  float *hst = p.hstate + ((size_t)dir * p.B + b) * H;
  float *o_ = p.out + row * 2 * H + (size_t)dir * H;
  for (int i = tid; i < H; i += NT) {
    const float chat = (cr[i] - meanc) * rc;
    const float c = fmaf(p.gamma[dir][4][i], chat, p.beta[dir][4][i]);
    const float h = tanhf_(c) * zs[3 * H + i];
    if (p.save) p.ch[dir][row * H + i] = chat;
    cst[i] = c;
    hst[i] = h;
    o_[i] = h;
  }
  if (p.save && tid < 4) p.rstd[dir][row * 4 + tid] = rs[tid];
  if (p.save && tid == 4) p.rstdc[dir][row] = rc;
}

// ---------------------------------------------------------------------------
// backward, launch 1 of a step: dh[b,u] = sum_col dz_{s+1}[b,col] · Wh[u,col]  (lstm_step_bwd_kernel's product)
__global__ __launch_bounds__(NT) void ln_rec_bwd_kernel(LnArgs p, int s) {
  __shared__ __attribute__((aligned(16))) float dzs[SB][DZC];
  const int H = p.H, B = p.B, T = p.T;
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int tid = threadIdx.x;
  const int u = tid & 15, bl = tid >> 4;
  const int b = b0 + bl, hu = u0 + u;
  const bool valid = b < B && hu < H;

  float dh = 0.f;
  const float *Wrow = p.kernel[dir] + (size_t)(p.D + (hu < H ? hu : 0)) * 4 * H;
  for (int c0 = 0; c0 < 4 * H; c0 += DZC) {
    const int cw = min(DZC, 4 * H - c0);
    __syncthreads();
    for (int i = tid; i < SB * (DZC / 4); i += NT) {
      const int r = i / (DZC / 4), c4 = i % (DZC / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int bb = b0 + r;
      if (bb < B && 4 * c4 < cw) {
        const int nn = p.len[bb];
        if (s + 1 < nn) {
          const int t1 = dir ? nn - 2 - s : s + 1;
          v = *reinterpret_cast<const float4 *>(p.zh[dir] + ((size_t)bb * T + t1) * 4 * H + c0 + 4 * c4);
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
  if (valid) p.dh[((size_t)dir * B + b) * H + hu] = dh;
}

// backward, launch 2 of a step: one workgroup per (row b, direction); activations recomputed from z_hat, c_hat and the
// row's rstd.  LDS: xs [4H] z_hat | wk [4H] activations, then dy | chs [H] | cps [H] c_{s-1} | gsv [H] | red [32]
__global__ __launch_bounds__(NT) void ln_cell_bwd_kernel(LnArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, T = p.T;
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int n = p.len[b];
  if (s >= n) {   // padded frame s >= len: dz must be 0 for the weight-gradient products
    float4 *gp4 = reinterpret_cast<float4 *>(p.zh[dir] + ((size_t)b * T + s) * 4 * H);
    for (int i = tid; i < H; i += NT) gp4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float *xs = smem, *wk = smem + 4 * H, *chs = smem + 8 * H, *cps = smem + 9 * H, *gsv = smem + 10 * H,
        *red = smem + 11 * H;
  const int t = dir ? n - 1 - s : s;
  const size_t row = (size_t)b * T + t;
  float *gp = p.zh[dir] + row * 4 * H;
  const float invH = 1.0f / (float)H;
  const float *const *gam = p.gamma[dir];
  const float *const *bet = p.beta[dir];
  float *dcp = p.cstate + ((size_t)dir * p.B + b) * H;
  float *part = p.part + ((size_t)dir * p.B + b) * 10 * H;
  const float *dhp = p.dh + ((size_t)dir * p.B + b) * H;
  const float *dop = p.dout + row * 2 * H + (size_t)dir * H;
  const float *chp = p.ch[dir] + row * H;
  const float *chprev = s > 0 ? p.ch[dir] + ((size_t)b * T + (dir ? t + 1 : t - 1)) * H : nullptr;

  // the state norm: dc (w.r.t. the carried, normalised c) -> d c' (w.r.t. the cell's raw new state)
  float m[2] = {0.f, 0.f};
  for (int i = tid; i < H; i += NT) {
    float xh[4], a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xh[k] = gp[k * H + i];
      xs[k * H + i] = xh[k];
      a[k] = fmaf(gam[k][i], xh[k], bet[k][i]);
    }
    const float ig = sigmoidf_(a[0]), g = tanhf_(a[1]), f = sigmoidf_(a[2] + 1.0f), o = sigmoidf_(a[3]);
    const float chat = chp[i];
    const float gs = gam[4][i], bs = bet[4][i];
    const float tc = tanhf_(fmaf(gs, chat, bs));
    const float dht = dop[i] + (p.has_dh ? dhp[i] : 0.f);
    const float dcn = dcp[i] + dht * o * (1.f - tc * tc);
    wk[i] = ig; wk[H + i] = g; wk[2 * H + i] = f;
    wk[3 * H + i] = dht * tc * o * (1.f - o);          // dy of the output gate
    chs[i] = chat;
    cps[i] = chprev ? fmaf(gs, chprev[i], bs) : 0.f;
    const float gv = dcn * gs;
    gsv[i] = gv;
    part[4 * H + i] += dcn * chat;
    part[9 * H + i] += dcn;
    m[0] += gv;
    m[1] = fmaf(gv, chat, m[1]);
  }
  block_sum<2>(m, red);
  const float rc = p.rstdc[dir][row];
  const float m1 = m[0] * invH, m2 = m[1] * invH;

  float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < H; i += NT) {
    const float dcr = rc * (gsv[i] - m1 - chs[i] * m2);
    const float ig = wk[i], g = wk[H + i], f = wk[2 * H + i];
    float dy[4];
    dy[0] = dcr * g * ig * (1.f - ig);
    dy[1] = dcr * ig * (1.f - g * g);
    dy[2] = dcr * cps[i] * f * (1.f - f);
    dy[3] = wk[3 * H + i];
    dcp[i] = dcr * f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xh = xs[k * H + i];
      part[k * H + i] = fmaf(dy[k], xh, part[k * H + i]);
      part[(5 + k) * H + i] += dy[k];
      const float gv = dy[k] * gam[k][i];
      wk[k * H + i] = gv;
      q[k] += gv;
      q[4 + k] = fmaf(gv, xh, q[4 + k]);
    }
  }
  block_sum<8>(q, red);
  float rs[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { rs[k] = p.rstd[dir][row * 4 + k]; q[k] *= invH; q[4 + k] *= invH; }
  for (int i = tid; i < H; i += NT)
#pragma unroll
    for (int k = 0; k < 4; ++k) gp[k * H + i] = rs[k] * (wk[k * H + i] - q[k] - xs[k * H + i] * q[4 + k]);
}

// the norm-parameter gradients: the rows' sums added in ascending row order.  grid (ceil(H / 256), 10, 2)
struct LnGradOut { float *dgamma[2][5], *dbeta[2][5]; };
__global__ __launch_bounds__(NT) void ln_param_grad_kernel(const float *part, int B, int H, LnGradOut o) {
  const int i = blockIdx.x * NT + threadIdx.x, q = blockIdx.y, dir = blockIdx.z;
  if (i >= H) return;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) acc += part[(((size_t)dir * B + b) * 10 + q) * H + i];
  (q < 5 ? o.dgamma[dir][q] : o.dbeta[dir][q - 5])[i] = acc;
}

// ---------------------------------------------------------------------------
struct LnLayout {
  size_t zh_elems, ch_elems, rstd_elems, rstdc_elems, reserve_bytes;
  size_t hstate_off, cstate_off, dh_off, part_off, part_bytes, gemm_off, gemm_bytes, total;
  size_t shm_rec, shm_cell_fwd, shm_cell_bwd;
  bool fwd_only;
};
constexpr size_t LDS_MAX = 160 * 1024;   // gfx950: LDS of one workgroup

static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// the descriptor as nabu_blstm_fwd reads it (the three sizes of its history); the packed-companion fields are not looked at
static int load_desc(const nabu_blstm_desc *in, nabu_blstm_desc *out) {
  constexpr uint32_t V1 = 8 * sizeof(int32_t), V2 = 11 * sizeof(int32_t);
  if (!in || (in->size != sizeof(nabu_blstm_desc) && in->size != V1 && in->size != V2))
    return fail(NABU_EINVAL, "blstm_ln: bad descriptor size");
  *out = nabu_blstm_desc{};
  memcpy(out, in, in->size);
  out->size = sizeof(nabu_blstm_desc);
  const nabu_blstm_desc *d = out;
  if (d->flags & ~NABU_BLSTM_FWD_ONLY) return fail(NABU_EINVAL, "blstm_ln: unknown flag bits %d", d->flags);
  if (d->recurrent_precision != NABU_REC_DEFAULT && d->recurrent_precision != NABU_REC_F32)
    return fail(NABU_EINVAL, "blstm_ln: recurrent_precision must be NABU_REC_DEFAULT or NABU_REC_F32");
  if (d->B <= 0 || d->T <= 0 || d->D <= 0 || d->H <= 0) return fail(NABU_EINVAL, "blstm_ln: non-positive dimension");
  if (d->max_len < 0 || d->max_len > d->T) return fail(NABU_EINVAL, "blstm_ln: max_len out of range");
  if (d->mode != NABU_LSTM_AUTO && d->mode != NABU_LSTM_STEPWISE && d->mode != NABU_LSTM_PERSISTENT)
    return fail(NABU_EINVAL, "blstm_ln: unknown mode %d", d->mode);
  if (d->H % 4 != 0) return fail(NABU_EUNSUP, "blstm_ln: num_units must be a multiple of 4 (got %d)", d->H);
  if (d->mode == NABU_LSTM_PERSISTENT)
    return fail(NABU_EUNSUP, "blstm_ln: the persistent recurrent kernels split the units of a row over workgroups and have "
                "no per-step reduction across them — layer norm runs in the stepwise family (NABU_LSTM_AUTO or _STEPWISE)");
  const size_t H = d->H;
  if (max_sz((SB * H + SB * 4 * SU) * 4, (11 * H + 32) * 4) > LDS_MAX)
    return fail(NABU_EUNSUP, "blstm_ln: num_units %d does not fit a workgroup's LDS (a row of 16 H resp. 11 H floats)", d->H);
  return 0;
}

static LnLayout make_layout(const nabu_blstm_desc *d) {
  LnLayout L = {};
  const size_t B = d->B, T = d->T, D = d->D, H = d->H;
  L.fwd_only = (d->flags & NABU_BLSTM_FWD_ONLY) != 0;
  L.zh_elems = B * T * 4 * H;
  L.ch_elems = L.fwd_only ? 0 : B * T * H;
  L.rstd_elems = L.fwd_only ? 0 : B * T * 4;
  L.rstdc_elems = L.fwd_only ? 0 : B * T;
  L.reserve_bytes = 2 * (L.zh_elems + L.ch_elems + L.rstd_elems + L.rstdc_elems) * sizeof(float);
  size_t off = 0;
  const size_t st = align_up(2 * B * H * sizeof(float), 256);
  L.hstate_off = off; off += st;
  L.cstate_off = off; off += st;
  L.dh_off = off; off += st;
  L.part_bytes = 20 * B * H * sizeof(float);
  L.part_off = off; off += align_up(L.part_bytes, 256);
  const int M = (int)(B * T);
  size_t g = 0;
  g = max_sz(g, nabu_gemm_ws_bytes(M, (int)(4 * H), (int)D));            // x·Wx
  g = max_sz(g, nabu_gemm_ws_bytes(M, (int)D, (int)(4 * H)));            // dz·Wx^T
  g = max_sz(g, nabu_gemm_ws_bytes((int)D, (int)(4 * H), M));            // x^T·dz
  if (T > 1) g = max_sz(g, nabu_gemm_ws_bytes((int)H, (int)(4 * H), (int)(B * (T - 1))));
  L.gemm_off = off; L.gemm_bytes = align_up(g, 256); off += L.gemm_bytes;
  L.total = off;
  L.shm_rec = (SB * H + SB * 4 * SU) * sizeof(float);
  L.shm_cell_fwd = (5 * H + 16) * sizeof(float);
  L.shm_cell_bwd = (11 * H + 32) * sizeof(float);
  return L;
}

// the reserve contract of nabu_hip.h for these entry points: what the forward call wrote, keyed by the reserve's address
struct LnTag {
  const void *reserve;
  uint64_t serial;
  int32_t B, T, D, H, flags;
  size_t reserve_bytes;
};
static std::mutex g_tag_mutex;
static LnTag g_tags[1024];   // (the least recently written is replaced)
static uint64_t g_tag_serial = 0;
static void tag_store(const nabu_blstm_desc *d, const LnLayout &L, const void *reserve) {
  std::lock_guard<std::mutex> lock(g_tag_mutex);
  LnTag *slot = &g_tags[0];
  for (LnTag &e : g_tags) {
    if (e.reserve == reserve) { slot = &e; break; }
    if (e.serial < slot->serial) slot = &e;
  }
  *slot = LnTag{reserve, ++g_tag_serial, d->B, d->T, d->D, d->H, d->flags, L.reserve_bytes};
}
static int tag_check(const nabu_blstm_desc *d, const LnLayout &L, const void *reserve, const char *who) {
  if (L.fwd_only)
    return fail(NABU_EINVAL, "%s: the descriptor says NABU_BLSTM_FWD_ONLY — its reserve has no room for a backward pass", who);
  std::lock_guard<std::mutex> lock(g_tag_mutex);
  for (const LnTag &e : g_tags) {
    if (e.reserve != reserve || !e.serial) continue;
    if (e.B == d->B && e.T == d->T && e.D == d->D && e.H == d->H && e.flags == d->flags && e.reserve_bytes == L.reserve_bytes)
      return 0;
    return fail(NABU_EINVAL, "%s: the reserve was written by nabu_blstm_ln_fwd under another layout (B %d T %d D %d H %d, %zu "
                "bytes, flags %d; this call: B %d T %d D %d H %d, %zu bytes)", who, e.B, e.T, e.D, e.H, e.reserve_bytes, e.flags,
                d->B, d->T, d->D, d->H, L.reserve_bytes);
  }
  return fail(NABU_EINVAL, "%s: no nabu_blstm_ln_fwd call of this process wrote this reserve (%p)", who, reserve);
}

static int check_ln(const nabu_blstm_ln_params *ln, bool grads, const char *who) {
  if (!ln || ln->size != sizeof(nabu_blstm_ln_params)) return fail(NABU_EINVAL, "%s: bad nabu_blstm_ln_params size", who);
  for (int dir = 0; dir < 2; ++dir)
    for (int k = 0; k < 5; ++k) {
      if (!ln->gamma[dir][k] || !ln->beta[dir][k]) return fail(NABU_EINVAL, "%s: null gamma/beta pointer", who);
      if (grads && (!ln->dgamma[dir][k] || !ln->dbeta[dir][k])) return fail(NABU_EINVAL, "%s: null dgamma/dbeta pointer", who);
    }
  return 0;
}

static void fill_args(LnArgs &p, const nabu_blstm_desc *d, const LnLayout &L, const int32_t *len, const float *kernel_fw,
                      const float *kernel_bw, const nabu_blstm_ln_params *ln, void *reserve, void *ws) {
  p = LnArgs{};
  p.B = d->B; p.T = d->T; p.D = d->D; p.H = d->H; p.max_len = d->max_len > 0 ? d->max_len : d->T;
  p.save = L.fwd_only ? 0 : 1;
  p.len = len;
  p.kernel[0] = kernel_fw; p.kernel[1] = kernel_bw;
  float *r = static_cast<float *>(reserve);
  p.zh[0] = r; p.zh[1] = r + L.zh_elems; r += 2 * L.zh_elems;
  p.ch[0] = r; p.ch[1] = r + L.ch_elems; r += 2 * L.ch_elems;
  p.rstd[0] = r; p.rstd[1] = r + L.rstd_elems; r += 2 * L.rstd_elems;
  p.rstdc[0] = r; p.rstdc[1] = r + L.rstdc_elems;
  if (ln)
    for (int dir = 0; dir < 2; ++dir)
      for (int k = 0; k < 5; ++k) { p.gamma[dir][k] = ln->gamma[dir][k]; p.beta[dir][k] = ln->beta[dir][k]; }
  char *w = static_cast<char *>(ws);
  p.hstate = reinterpret_cast<float *>(w + L.hstate_off);
  p.cstate = reinterpret_cast<float *>(w + L.cstate_off);
  p.dh = reinterpret_cast<float *>(w + L.dh_off);
  p.part = reinterpret_cast<float *>(w + L.part_off);
}

template <typename K>
static int allow_lds(K kernel, size_t shm) {
  if (shm > 64 * 1024)
    NABU_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  return 0;
}

// parts: 1 = data (recurrence backwards, norm-parameter gradients, d_x), 2 = weights (dkernel from the dz in the reserve)
static int ln_bwd_parts(int parts, const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *kernel_fw,
                        const float *kernel_bw, const nabu_blstm_ln_params *ln, const float *out, const float *d_out,
                        void *reserve, float *d_x, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                        nabu_stream_t stream) {
  const char *who = parts == 3 ? "blstm_ln_bwd" : parts == 1 ? "blstm_ln_bwd_data" : "blstm_ln_bwd_weights";
  NABU_CHECK_ARG(x && len && out && reserve && ws, "%s: null pointer", who);
  if (parts & 1) {
    NABU_CHECK_ARG(kernel_fw && kernel_bw && d_out, "%s: null pointer", who);
    if (int e = check_ln(ln, true, who)) return e;
  }
  if (parts & 2) NABU_CHECK_ARG(dkernel_fw && dkernel_bw, "%s: null pointer", who);
  const LnLayout L = make_layout(d);
  if (int e = tag_check(d, L, reserve, who)) return e;
  if (ws_bytes < L.total) return fail(NABU_EWS, "%s: workspace %zu < %zu", who, ws_bytes, L.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int B = d->B, T = d->T, D = d->D, H = d->H, M = B * T;
  LnArgs p;
  fill_args(p, d, L, len, kernel_fw, kernel_bw, (parts & 1) ? ln : nullptr, reserve, ws);
  char *w = static_cast<char *>(ws);

  if (parts & 1) {
    p.dout = d_out;
    // dz rows of frames never visited by the recurrence must be zero
    if (p.max_len < T)
      for (int dir = 0; dir < 2; ++dir)
        NABU_HIP(hipMemset2DAsync(p.zh[dir] + (size_t)p.max_len * 4 * H, (size_t)T * 4 * H * sizeof(float), 0,
                                  (size_t)(T - p.max_len) * 4 * H * sizeof(float), B, s));
    NABU_HIP(hipMemsetAsync(p.cstate, 0, 2 * (size_t)B * H * sizeof(float), s));
    NABU_HIP(hipMemsetAsync(p.part, 0, L.part_bytes, s));
    if (int e = allow_lds(ln_cell_bwd_kernel, L.shm_cell_bwd)) return e;
    const dim3 grid_rec((H + SU - 1) / SU, (B + SB - 1) / SB, 2), grid_cell(B, 2);
    for (int t = p.max_len - 1; t >= 0; --t) {
      p.has_dh = t + 1 < p.max_len;
      if (p.has_dh) hipLaunchKernelGGL(ln_rec_bwd_kernel, grid_rec, dim3(NT), 0, s, p, t);
      hipLaunchKernelGGL(ln_cell_bwd_kernel, grid_cell, dim3(NT), L.shm_cell_bwd, s, p, t);
    }
    LnGradOut go;
    for (int dir = 0; dir < 2; ++dir)
      for (int k = 0; k < 5; ++k) { go.dgamma[dir][k] = ln->dgamma[dir][k]; go.dbeta[dir][k] = ln->dbeta[dir][k]; }
    hipLaunchKernelGGL(ln_param_grad_kernel, dim3((H + NT - 1) / NT, 10, 2), dim3(NT), 0, s, p.part, B, H, go);
    NABU_LAUNCH_CHECK();
    // dx = dz_fw · Wx_fw^T + dz_bw · Wx_bw^T
    if (d_x)
      for (int dir = 0; dir < 2; ++dir)
        if (int e = nabu_gemm_ex(d->gemm_precision, 0, 1, M, D, 4 * H, 1.f, p.zh[dir], 4 * H, p.kernel[dir], 4 * H,
                                 dir == 0 ? 0.f : 1.f, d_x, D, nullptr, 0, 0, 0, w + L.gemm_off, L.gemm_bytes, stream))
          return e;
  }
  if (parts & 2) {
    float *dkern[2] = {dkernel_fw, dkernel_bw};
    for (int dir = 0; dir < 2; ++dir) {
      // dWx = x^T · dz
      if (int e = nabu_gemm_ex(d->gemm_precision, 1, 0, D, 4 * H, M, 1.f, x, D, p.zh[dir], 4 * H, 0.f, dkern[dir], 4 * H,
                               nullptr, 0, 0, 0, w + L.gemm_off, L.gemm_bytes, stream))
        return e;
      // dWh = h_{prev}^T · dz : fw pairs (out[b,t-1,:H], dz[b,t]); bw pairs (out[b,t+1,H:], dz[b,t])
      float *dWh = dkern[dir] + (size_t)D * 4 * H;
      if (T == 1) {
        NABU_HIP(hipMemsetAsync(dWh, 0, (size_t)H * 4 * H * sizeof(float), s));
        continue;
      }
      const float *A = dir == 0 ? out : out + H + (size_t)2 * H;
      const float *Bm = dir == 0 ? p.zh[0] + (size_t)4 * H : p.zh[1];
      if (int e = nabu_gemm_f32(1, 0, H, 4 * H, B * (T - 1), 1.f, A, 2 * H, Bm, 4 * H, 0.f, dWh, 4 * H, nullptr, T - 1,
                                (long long)T * 2 * H, (long long)T * 4 * H, w + L.gemm_off, L.gemm_bytes, stream))
        return e;
    }
  }
  return 0;
}

}  // namespace
}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_blstm_ln_reserve_bytes(const nabu_blstm_desc *d_in) {
  nabu_blstm_desc d;
  if (load_desc(d_in, &d)) return 0;
  return make_layout(&d).reserve_bytes;
}
extern "C" size_t nabu_blstm_ln_ws_bytes(const nabu_blstm_desc *d_in) {
  nabu_blstm_desc d;
  if (load_desc(d_in, &d)) return 0;
  return make_layout(&d).total;
}

extern "C" int nabu_blstm_ln_fwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *kernel_fw,
                                 const float *kernel_bw, const nabu_blstm_ln_params *ln, float *out, void *reserve,
                                 void *ws, size_t ws_bytes, nabu_stream_t stream) {
  nabu_blstm_desc dd;
  if (int e = load_desc(d_in, &dd)) return e;
  const nabu_blstm_desc *d = &dd;
  NABU_CHECK_ARG(x && len && kernel_fw && kernel_bw && out && reserve && ws, "blstm_ln_fwd: null pointer");
  if (int e = check_ln(ln, false, "blstm_ln_fwd")) return e;
  const LnLayout L = make_layout(d);
  if (ws_bytes < L.total) return fail(NABU_EWS, "blstm_ln_fwd: workspace %zu < %zu", ws_bytes, L.total);
  tag_store(d, L, reserve);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int B = d->B, T = d->T, D = d->D, H = d->H;
  LnArgs p;
  fill_args(p, d, L, len, kernel_fw, kernel_bw, ln, reserve, ws);
  p.out = out;
  char *w = static_cast<char *>(ws);
  // time-batched input projections: zh_d = x · Wx_d (the cell has no bias)
  for (int dir = 0; dir < 2; ++dir)
    if (int e = nabu_gemm_ex(d->gemm_precision, 0, 0, B * T, 4 * H, D, 1.f, x, D, p.kernel[dir], 4 * H, 0.f, p.zh[dir], 4 * H,
                             nullptr, 0, 0, 0, w + L.gemm_off, L.gemm_bytes, stream))
      return e;
  // frames t in [max_len, T) are never visited by the recurrence
  if (p.max_len < T)
    NABU_HIP(hipMemset2DAsync(out + (size_t)p.max_len * 2 * H, (size_t)T * 2 * H * sizeof(float), 0,
                              (size_t)(T - p.max_len) * 2 * H * sizeof(float), B, s));
  NABU_HIP(hipMemsetAsync(p.hstate, 0, 2 * (size_t)B * H * sizeof(float), s));
  NABU_HIP(hipMemsetAsync(p.cstate, 0, 2 * (size_t)B * H * sizeof(float), s));
  if (int e = allow_lds(ln_rec_fwd_kernel, L.shm_rec)) return e;
  if (int e = allow_lds(ln_cell_fwd_kernel, L.shm_cell_fwd)) return e;
  const dim3 grid_rec((H + SU - 1) / SU, (B + SB - 1) / SB, 2), grid_cell(B, 2);
  for (int t = 0; t < p.max_len; ++t) {
    if (t > 0) hipLaunchKernelGGL(ln_rec_fwd_kernel, grid_rec, dim3(NT), L.shm_rec, s, p, t);   // (h_{-1} = 0: z is x·Wx)
    hipLaunchKernelGGL(ln_cell_fwd_kernel, grid_cell, dim3(NT), L.shm_cell_fwd, s, p, t);
  }
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_blstm_ln_bwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *kernel_fw,
                                 const float *kernel_bw, const nabu_blstm_ln_params *ln, const float *out,
                                 const float *d_out, void *reserve, float *d_x, float *dkernel_fw, float *dkernel_bw,
                                 void *ws, size_t ws_bytes, nabu_stream_t stream) {
  nabu_blstm_desc d;
  if (int e = load_desc(d_in, &d)) return e;
  return ln_bwd_parts(3, &d, x, len, kernel_fw, kernel_bw, ln, out, d_out, reserve, d_x, dkernel_fw, dkernel_bw, ws, ws_bytes,
                      stream);
}
extern "C" int nabu_blstm_ln_bwd_data(const nabu_blstm_desc *d_in, const float *x, const int32_t *len,
                                      const float *kernel_fw, const float *kernel_bw, const nabu_blstm_ln_params *ln,
                                      const float *out, const float *d_out, void *reserve, float *d_x, void *ws,
                                      size_t ws_bytes, nabu_stream_t stream) {
  nabu_blstm_desc d;
  if (int e = load_desc(d_in, &d)) return e;
  return ln_bwd_parts(1, &d, x, len, kernel_fw, kernel_bw, ln, out, d_out, reserve, d_x, nullptr, nullptr, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_ln_bwd_weights(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *out,
                                         void *reserve, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                                         nabu_stream_t stream) {
  nabu_blstm_desc d;
  if (int e = load_desc(d_in, &d)) return e;
  return ln_bwd_parts(2, &d, x, len, nullptr, nullptr, nullptr, out, nullptr, reserve, nullptr, dkernel_fw, dkernel_bw, ws,
                      ws_bytes, stream);
}
