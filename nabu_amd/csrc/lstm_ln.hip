// lstm_ln.hip — the recurrence of a bidirectional LSTM layer with layer normalisation inside the cell
// (layer.blstm(layer_norm=True), tf.contrib.rnn.LayerNormBasicLSTMCell(layer_norm=True); the semantics are stated in
// include/nabu_hip.h).  The layer around it — descriptor, reserve contract, dense products — is lstm.hip's driver.
//
// The exact-fp32, launch-per-step family: the row statistics of a step need all H units of a row, so a step is TWO
// launches, both directions in each:
//   forward   ln_rec_fwd_kernel   z[b,t] += h_{s-1} · Wh            grid (H/16, B/16, 2)  (rec_fwd_tile, lstm_step.h)
//             ln_cell_fwd_kernel  statistics, gates, state norm, h   grid (B, 2): one workgroup per row and direction
//   backward  ln_rec_bwd_kernel   dh = dz_{s+1} · Wh^T              grid (H/16, B/16, 2)  (rec_bwd_tile)
//             ln_cell_bwd_kernel  cell and norm gradients, dz        grid (B, 2)
// Row statistics: two-pass (mean, then the centred squares) sums of 256 threads — a butterfly inside each wave, the four
// wave sums added in one fixed order.  The gamma/beta gradients are running sums per (direction, row) in the workspace,
// each owned by the one workgroup of that row, and are added over the rows in ascending order by one launch behind the
// recurrence: no floating-point atomics anywhere.
//
// reserve (fp32, batch-major):
//   gates_fw | gates_bw [B,T,4H]   x·Wx (GEMM output), then z (ln_rec_fwd), then the normalised z_hat (ln_cell_fwd), then dz —
//                            the gradient w.r.t. the pre-normalisation z (ln_cell_bwd); all in place
//   cs_fw | cs_bw [B,T,H]    the normalised new cell state before gamma/beta (stands where the plain cell keeps cs)
//   rstd_fw | rstd_bw [B,T,4], rstdc_fw | rstdc_bw [B,T]
// A forward-only call uses the gate buffers alone and writes nothing back into them behind z.
#include "lstm_step.h"

namespace nabu {
namespace {

constexpr float LN_EPS = 1e-12f;
constexpr int NT = STEP_NT;

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
// forward, launch 1 of a step: z[b,t] += h_{s-1}[b] · Wh for the rows still running
__global__ __launch_bounds__(NT) void ln_rec_fwd_kernel(LnArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, B = p.B, T = p.T;
  float *hs = smem;               // [SB][H]
  float *zs = smem + SB * H;      // [SB][4][SU]
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int tid = threadIdx.x;
  rec_fwd_tile(p, p.hstate + (size_t)dir * B * H, dir, b0, u0, hs, zs);
  {  // thread = (batch row bl, unit u)
    const int u = tid & 15, bl = tid >> 4;
    const int b = b0 + bl, hu = u0 + u;
    if (b < B && hu < H) {
      const int n = p.len[b];
      if (s < n) {
        const int t = dir ? n - 1 - s : s;
        float *gp = p.gates[dir] + ((size_t)b * T + t) * 4 * H + hu;
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
  float *gp = p.gates[dir] + row * 4 * H;
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
    if (p.save) p.cs[dir][row * H + i] = chat;
    cst[i] = c;
    hst[i] = h;
    o_[i] = h;
  }
  if (p.save && tid < 4) p.rstd[dir][row * 4 + tid] = rs[tid];
  if (p.save && tid == 4) p.rstdc[dir][row] = rc;
}

// ---------------------------------------------------------------------------
// backward, launch 1 of a step: dh[b,u] = sum_col dz_{s+1}[b,col] · Wh[u,col]
__global__ __launch_bounds__(NT) void ln_rec_bwd_kernel(LnArgs p, int s) {
  __shared__ __attribute__((aligned(16))) float dzs[SB][DZC];
  const int H = p.H, B = p.B;
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int b = b0 + (threadIdx.x >> 4), hu = u0 + (threadIdx.x & 15);
  const float dh = rec_bwd_tile(p, dir, s, b0, u0, dzs);
  if (b < B && hu < H) p.dh[((size_t)dir * B + b) * H + hu] = dh;
}

// backward, launch 2 of a step: one workgroup per (row b, direction); activations recomputed from z_hat, c_hat and the
// row's rstd.  LDS: xs [4H] z_hat | wk [4H] activations, then dy | chs [H] | cps [H] c_{s-1} | gsv [H] | red [32]
__global__ __launch_bounds__(NT) void ln_cell_bwd_kernel(LnArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, T = p.T;
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int n = p.len[b];
  if (s >= n) {   // padded frame s >= len: dz must be 0 for the weight-gradient products
    float4 *gp4 = reinterpret_cast<float4 *>(p.gates[dir] + ((size_t)b * T + s) * 4 * H);
    for (int i = tid; i < H; i += NT) gp4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float *xs = smem, *wk = smem + 4 * H, *chs = smem + 8 * H, *cps = smem + 9 * H, *gsv = smem + 10 * H,
        *red = smem + 11 * H;
  const int t = dir ? n - 1 - s : s;
  const size_t row = (size_t)b * T + t;
  float *gp = p.gates[dir] + row * 4 * H;
  const float invH = 1.0f / (float)H;
  const float *const *gam = p.gamma[dir];
  const float *const *bet = p.beta[dir];
  float *dcp = p.cstate + ((size_t)dir * p.B + b) * H;
  float *part = p.part + ((size_t)dir * p.B + b) * 10 * H;
  const float *dhp = p.dh + ((size_t)dir * p.B + b) * H;
  const float *dop = p.dout + row * 2 * H + (size_t)dir * H;
  const float *chp = p.cs[dir] + row * H;
  const float *chprev = s > 0 ? p.cs[dir] + ((size_t)b * T + (dir ? t + 1 : t - 1)) * H : nullptr;

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
static size_t shm_rec(size_t H) { return (SB * H + SB * 4 * SU) * sizeof(float); }
static size_t shm_cell_fwd(size_t H) { return (5 * H + 16) * sizeof(float); }
static size_t shm_cell_bwd(size_t H) { return (11 * H + 32) * sizeof(float); }
static dim3 grid_rec(const LnArgs &p) { return dim3((p.H + SU - 1) / SU, (p.B + SB - 1) / SB, 2); }

}  // namespace

size_t ln_lds_bytes(int H) { return shm_rec(H) > shm_cell_bwd(H) ? shm_rec(H) : shm_cell_bwd(H); }

int ln_recurrence_fwd(LnArgs p, hipStream_t s) {
  NABU_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(ln_rec_fwd_kernel), shm_rec(p.H)));
  NABU_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(ln_cell_fwd_kernel), shm_cell_fwd(p.H)));
  for (int t = 0; t < p.max_len; ++t) {
    if (t > 0) hipLaunchKernelGGL(ln_rec_fwd_kernel, grid_rec(p), dim3(NT), shm_rec(p.H), s, p, t);   // (h_{-1} = 0: z is x·Wx)
    hipLaunchKernelGGL(ln_cell_fwd_kernel, dim3(p.B, 2), dim3(NT), shm_cell_fwd(p.H), s, p, t);
  }
  NABU_LAUNCH_CHECK();
  return 0;
}

int ln_recurrence_bwd(LnArgs p, hipStream_t s) {
  NABU_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(ln_cell_bwd_kernel), shm_cell_bwd(p.H)));
  for (int t = p.max_len - 1; t >= 0; --t) {
    p.has_dh = t + 1 < p.max_len;
    if (p.has_dh) hipLaunchKernelGGL(ln_rec_bwd_kernel, grid_rec(p), dim3(NT), 0, s, p, t);
    hipLaunchKernelGGL(ln_cell_bwd_kernel, dim3(p.B, 2), dim3(NT), shm_cell_bwd(p.H), s, p, t);
  }
  return 0;
}

int ln_param_grads(const LnArgs &p, const nabu_blstm_ln_params *ln, hipStream_t s) {
  LnGradOut go;
  for (int dir = 0; dir < 2; ++dir)
    for (int k = 0; k < 5; ++k) { go.dgamma[dir][k] = ln->dgamma[dir][k]; go.dbeta[dir][k] = ln->dbeta[dir][k]; }
  hipLaunchKernelGGL(ln_param_grad_kernel, dim3((p.H + NT - 1) / NT, 10, 2), dim3(NT), 0, s, p.part, p.B, p.H, go);
  NABU_LAUNCH_CHECK();
  return 0;
}

}  // namespace nabu
