// lstm.hip — one bidirectional LSTM layer (layer.blstm of the reference), for both cells: the plain cell
// (nabu_blstm_*) and the layer-normalised one (nabu_blstm_ln_*, layer.blstm(layer_norm=True)).  The entry points are
// adapters around ONE forward and ONE backward driver that take the cell as an argument and read as a sequence of stages:
//   forward   input projection (packed-plane operands | plain) · zeroing of frames >= max_len · companions ·
//             recurrence (persistent, with its fallback | stepwise plain | stepwise layer-norm)
//   backward  zeroing · recurrence · norm-parameter gradients · packed products · plain products and bias gradients
// What the layer-normalised cell does NOT take (packed products, bias, companions, a persistent plan, the profiling
// hooks) is decided in one place, ln_layout; the stages read the layout.  The plain cell's step kernels are here, the
// layer-normalised cell's in lstm_ln.hip; both use the product tiles of lstm_step.h.
//
// Data layout in HBM (all fp32, batch-major):
//   x      [B,T,D]        layer input
//   out    [B,T,2H]       fw | bw hidden states, 0 for t >= len
//   reserve = gates_fw [B,T,4H] | gates_bw [B,T,4H] | cs_fw [B,T,H] | cs_bw [B,T,H]   (layer norm: lstm_ln.hip)
//     gates_* first holds x·Wx+b (GEMM output), is overwritten in place by the
//     activations (i,g,f,o) in the forward recurrence and again in place by the
//     pre-activation gradients dz in the backward recurrence.
// The TF kernel [(D+H),4H] is used as stored: rows [0,D) = Wx, rows [D,D+H) = Wh.
#include "common.h"
#include "lstm_persist.h"
#include "lstm_step.h"

#include <stdlib.h>
#include <string.h>
#include <mutex>
#include "gemm_args.h"

namespace nabu {

struct StepArgs {
  int B, T, D, H, max_len;
  const int32_t *len;
  const float *kernel[2];  // per direction
  float *gates[2];
  float *cs[2];
  float *out;          // fwd: written; bwd: unused
  const float *dout;   // bwd
  float *hstate;       // [2 pingpong][2 dir][B][H]
  float *cstate;       // fwd: c state [2][B][H]; bwd: dc carry [2][B][H]
};

// ---------------------------------------------------------------------------
// forward, one timestep, both directions.  grid (H/16, B/16, 2), 256 threads.
__global__ __launch_bounds__(STEP_NT) void lstm_step_fwd_kernel(StepArgs p, int s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = p.H, B = p.B, T = p.T;
  float *hs = smem;               // [SB][H]
  float *zs = smem + SB * H;      // [SB][4][SU]
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int tid = threadIdx.x;
  // the cell is fused behind the product: h ping-pongs between two buffers
  const float *hprev = p.hstate + ((size_t)((s & 1) * 2 + dir) * B) * H;
  float *hnext = p.hstate + ((size_t)(((s & 1) ^ 1) * 2 + dir) * B) * H;
  rec_fwd_tile(p, hprev, dir, b0, u0, hs, zs);

  {  // gates + state update: thread = (batch row bl, unit u)
    const int u = tid & 15, bl = tid >> 4;
    const int b = b0 + bl, hu = u0 + u;
    if (b < B && hu < H) {
      const int n = p.len[b];
      const size_t sidx = (size_t)b * H + hu;
      if (s < n) {
        const int t = dir ? n - 1 - s : s;
        float *gp = p.gates[dir] + ((size_t)b * T + t) * 4 * H + hu;
        const float zi = gp[0] + zs[(bl * 4 + 0) * SU + u];
        const float zj = gp[H] + zs[(bl * 4 + 1) * SU + u];
        const float zf = gp[2 * H] + zs[(bl * 4 + 2) * SU + u];
        const float zo = gp[3 * H] + zs[(bl * 4 + 3) * SU + u];
        const float i = sigmoidf_(zi), g = tanhf_(zj), f = sigmoidf_(zf + 1.0f), o = sigmoidf_(zo);
        float *cst = p.cstate + (size_t)dir * B * H + sidx;
        const float c = *cst * f + i * g;
        const float h = tanhf_(c) * o;
        gp[0] = i; gp[H] = g; gp[2 * H] = f; gp[3 * H] = o;
        p.cs[dir][((size_t)b * T + t) * H + hu] = c;
        p.out[((size_t)b * T + t) * 2 * H + (size_t)dir * H + hu] = h;
        *cst = c;
        hnext[sidx] = h;
      } else {
        // finished sequence: state frozen, output row s is zero (t >= len)
        hnext[sidx] = hs[bl * H + hu];
        p.out[((size_t)b * T + s) * 2 * H + (size_t)dir * H + hu] = 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward, one timestep (s descending), both directions.
//   dh_carry[b,u] = sum_col dz_{s+1}[b,col] * Wh[u,col]      (block-local)
//   dz_s from saved activations, written in place over the activations.
__global__ __launch_bounds__(STEP_NT) void lstm_step_bwd_kernel(StepArgs p, int s) {
  __shared__ __attribute__((aligned(16))) float dzs[SB][DZC];
  const int H = p.H, B = p.B, T = p.T;
  const int dir = blockIdx.z, u0 = blockIdx.x * SU, b0 = blockIdx.y * SB;
  const int tid = threadIdx.x;
  const int u = tid & 15, bl = tid >> 4;
  const int b = b0 + bl, hu = u0 + u;
  const bool valid = b < B && hu < H;
  const int n = b < B ? p.len[b] : 0;

  float dh = 0.f;
  if (s + 1 < p.max_len)
    dh = rec_bwd_tile(p, dir, s, b0, u0, dzs);
  if (!valid) return;
  if (s < n) {
    const int t = dir ? n - 1 - s : s;
    float *gp = p.gates[dir] + ((size_t)b * T + t) * 4 * H + hu;
    const float i = gp[0], g = gp[H], f = gp[2 * H], o = gp[3 * H];
    const float c = p.cs[dir][((size_t)b * T + t) * H + hu];
    float cprev = 0.f;
    if (s > 0) cprev = p.cs[dir][((size_t)b * T + (dir ? t + 1 : t - 1)) * H + hu];
    float *dcp = p.cstate + (size_t)dir * B * H + (size_t)b * H + hu;
    const float tc = tanhf_(c);
    const float dht = p.dout[((size_t)b * T + t) * 2 * H + (size_t)dir * H + hu] + dh;
    const float dct = *dcp + dht * o * (1.f - tc * tc);
    gp[0] = dct * g * i * (1.f - i);
    gp[H] = dct * i * (1.f - g * g);
    gp[2 * H] = dct * cprev * f * (1.f - f);
    gp[3 * H] = dht * tc * o * (1.f - o);
    *dcp = dct * f;
  } else {
    // padded frame s >= len: dz must be 0 for the weight-gradient GEMMs
    float *gp = p.gates[dir] + ((size_t)b * T + s) * 4 * H + hu;
    gp[0] = 0.f; gp[H] = 0.f; gp[2 * H] = 0.f; gp[3 * H] = 0.f;
  }
}

// ---------------------------------------------------------------------------
struct Layout {
  size_t gates_elems, cs_elems;
  size_t reserve_bytes;
  // workspace carve
  size_t hstate_off, cstate_off, gemm_off, gemm_bytes, persist_off, persist_bytes, xws_off, xws_bytes, total;
  PersistPlan plan;   // the persistent recurrence's launch plan for this call (lstm_persist.h): decided here, once
  // packed bf16-plane operands (gemm_pk.hip): planes = 3 (bf16x6) or 1 (bf16); pk_in = the input products
  // X·Wx, dZ·Wx^T, X^T·dZ, pk_rec = the recurrent weight gradient h_{t-1}^T·dZ
  int pk_planes;
  bool pk_in, pk_rec;
  bool pk_xw;       // the forward product X·Wx: pk_in, or plain bf16 below 256 inputs as well (cfg5's first layer: D = 80)
  bool pk_whole;    // narrow input (D < 256): [x^T ; h^T] is ONE operand and the whole kernel gradient one product
  size_t pk_off, pk_bytes;
  // forward: X [BT, D], W^T of both cells [8H, D]; backward: dZ^T [8H, BT], X^T [D, BT], h^T per cell [H, BT],
  // dZ [BT, 8H], Wx of both cells [D, 8H] (byte offsets inside the pk region)
  size_t pk_x, pk_w, pk_xT, pk_hT[2], pk_dz, pk_w2;
  // planes = 2 (f16x3): the row maxima (uint32 per packed row) of the operands above; those of one pass are
  // contiguous (one memset): forward [x | w], backward [dz | w2 | xT | hT0 | hT1]; dZ^T's sit behind it in the reserve
  // the column maxima of x and the row maxima of Wx (the backward pass's x^T and Wx operands) are measured by the
  // forward pass in the same reads as its own and kept in the reserve (res_axT_off, res_aw2_off)
  size_t pk_ax, pk_aw, pk_adz, pk_ahT[2], pk_abwd_bytes, res_adzT_off, res_axT_off, res_aw2_off;
  size_t res_xT_off;         // 0: none.  x^T as a packed operand (the weight-gradient product's), written by the forward
                             // call from the read of x that packs its own operand (one pass over x less per step)
  size_t res_ahT_off;        // 0: none.  The known row bound of h^T (|h| <= 1), written by the forward call's one fill
  bool x_colmax_kept;        // the whole-kernel form on f16x3 operands: EVERY forward call leaves the columns' maxima of x
                             // at res_axT_off (a region this form has no other use for) — the backward pass's row maxima
                             // of x^T.  A forward launch that reads x as planes measures them for its own scale anyway
                             // (one measurement per step); any other forward path measures them behind its recurrence.
                             // Decided by fields the reserve tag records (planes, pk_whole, flags) and a switch read
                             // once per process: never by the mode or the launch plan, which may differ between the passes
  // per-workgroup row maxima of dz written by the persistent backward kernel ([2 directions x H / 16][BT] bit patterns;
  // 0 bytes where the layer has no input gradient): the row scales of dZ as [BT, 8H] without a pass over dz
  size_t pk_rowmax, pk_rowmax_bytes;
  bool fwd_only;    // NABU_BLSTM_FWD_ONLY: the reserve ends behind the activations
  // ABI version 3, packed companions (include/nabu_hip.h): x_pk = the input operands come packed from the caller;
  // hT_ext = h^T lives in the caller's hT_pk, written by the forward call; cmp_* = sizes (nabu_blstm_pk_bytes) and a
  // scratch array of row maxima (all 1.0f) for the pack-kernel fallback
  bool x_pk, hT_ext;
  int out_stack;
  size_t cmp_bytes[5];
  size_t cmp_amax_off, cmp_amax_bytes;
  // dZ^T packed [8H, BT] lives in the layer's RESERVE (behind the activations): it is written by the data part of
  // the backward pass and read by the weight-gradient part, which may run later (nabu_blstm_bwd_weights)
  size_t res_dzT_off, res_dzT_bytes;
  // the layer-normalised cell (ln_layout): its statistics in the reserve behind cs (which holds the normalised state)
  // and, in the workspace, the recurrent product's dh and the per-row sums of the norm-parameter gradients
  bool ln;
  size_t rstd_elems, rstdc_elems, dh_off, part_off, part_bytes;
  size_t hstate_bytes;   // of the stepwise kernels' h state: ping-pong [2][2][B][H] (plain), [2][B][H] (layer norm)
  bool hooks;            // the profile events and the phase hook fire in this call
};

// ---------------------------------------------------------------------------
// THE DESCRIPTOR as every entry point reads it: ABI version 1 callers pass the 32-byte descriptor (everything up to
// gemm_precision), version 2 callers 44 bytes: the later fields read as 0.  The common checks, then those of the family.
// (The layer-normalised entry points do not look at the packed-companion fields, x_bound and out_stack.)
constexpr size_t LDS_MAX = 160 * 1024;   // gfx950: LDS of one workgroup
static int check_units(const nabu_blstm_desc *d, const char *who) {
  return d->H % 4 != 0 ? fail(NABU_EUNSUP, "%s: num_units must be a multiple of 4 (got %d)", who, d->H) : 0;
}
static int check_max_len(const nabu_blstm_desc *d, const char *who) {
  return d->max_len < 0 || d->max_len > d->T ? fail(NABU_EINVAL, "%s: max_len out of range", who) : 0;
}
static int load_desc(const nabu_blstm_desc *in, nabu_blstm_desc *out, bool ln) {
  const char *who = ln ? "blstm_ln" : "blstm";
  constexpr uint32_t V1 = 8 * sizeof(int32_t), V2 = 11 * sizeof(int32_t);
  if (!in || (in->size != sizeof(nabu_blstm_desc) && in->size != V1 && in->size != V2))
    return fail(NABU_EINVAL, "%s: bad descriptor size", who);
  *out = nabu_blstm_desc{};
  memcpy(out, in, in->size);
  out->size = sizeof(nabu_blstm_desc);
  nabu_blstm_desc *d = out;
  if (d->flags & ~NABU_BLSTM_FWD_ONLY) return fail(NABU_EINVAL, "%s: unknown flag bits %d", who, d->flags);
  if (d->recurrent_precision != NABU_REC_DEFAULT && d->recurrent_precision != NABU_REC_F32)
    return fail(NABU_EINVAL, "%s: recurrent_precision must be NABU_REC_DEFAULT or NABU_REC_F32", who);
  if (d->B <= 0 || d->T <= 0 || d->D <= 0 || d->H <= 0) return fail(NABU_EINVAL, "%s: non-positive dimension", who);
  if (!ln) {
    if (!(d->x_bound >= 0.f) || d->x_bound > 3.0e38f) return fail(NABU_EINVAL, "blstm: x_bound must be finite and >= 0");
    if (d->out_stack < 0 || d->out_stack > 2) return fail(NABU_EINVAL, "blstm: out_stack must be 0, 1 or 2");
    if (d->out_stack == 0) d->out_stack = 1;
    if ((d->x_pk_rows == nullptr) != (d->x_pk_cols == nullptr) && !(d->flags & NABU_BLSTM_FWD_ONLY))
      return fail(NABU_EINVAL, "blstm: x_pk_rows and x_pk_cols come as a pair (a forward-only descriptor may give the rows alone)");
    NABU_TRY(check_units(d, who));
    return check_max_len(d, who);
  }
  d->recurrent_precision = NABU_REC_DEFAULT;     // nothing of this family depends on it (nor the reserve's tag)
  NABU_TRY(check_max_len(d, who));
  if (d->mode != NABU_LSTM_AUTO && d->mode != NABU_LSTM_STEPWISE && d->mode != NABU_LSTM_PERSISTENT)
    return fail(NABU_EINVAL, "blstm_ln: unknown mode %d", d->mode);
  NABU_TRY(check_units(d, who));
  if (d->mode == NABU_LSTM_PERSISTENT)
    return fail(NABU_EUNSUP, "blstm_ln: the persistent recurrent kernels split the units of a row over workgroups and have "
                "no per-step reduction across them — layer norm runs in the stepwise family (NABU_LSTM_AUTO or _STEPWISE)");
  if (ln_lds_bytes(d->H) > LDS_MAX)
    return fail(NABU_EUNSUP, "blstm_ln: num_units %d does not fit a workgroup's LDS (a row of 16 H resp. 11 H floats)", d->H);
  return 0;
}
// every entry point works on the normalised copy
struct DescScope {
  nabu_blstm_desc d;
  bool ln;
  int err;
  DescScope(const nabu_blstm_desc *in, bool ln_) : ln(ln_), err(load_desc(in, &d, ln_)) {}
};
static PersistPlan plan_of(const nabu_blstm_desc *d) {
  return lstm_persist_plan(d->B, d->T, d->D, d->H, d->max_len > 0 ? d->max_len : d->T, d->recurrent_precision == NABU_REC_F32);
}

// planes of the packed-operand path for this layer (0 = not taken): bf16x6 -> 3, f16x3 -> 2, bf16 -> 1
static int pk_planes_of(const nabu_blstm_desc *d) {
  const int prec = d->gemm_precision == NABU_GEMM_DEFAULT ? nabu_gemm_get_default_precision() : d->gemm_precision;
  static const int env = env_int("NABU_PK", 1);
  if (!env || !gemm_pk_device_ok()) return 0;
  const long long BT = (long long)d->B * d->T;
  if (BT < 1024 || BT >= (1ll << 31) - 512 || d->H % 64) return 0;   // n_split = 4H must be a multiple of 256
  // f16x3 pays for its row maxima with ~20 small launches per layer and step: below 2048 frames (cfg1: 1600) the
  // other fp32-equivalent arithmetic is faster (2.06 against 2.16 ms per cfg1 step)
  if (prec == NABU_GEMM_F16X3) return BT >= 2048 ? 2 : 3;
  return prec == NABU_GEMM_BF16X6 ? 3 : prec == NABU_GEMM_BF16 ? 1 : 0;
}
// the row "maximum" an a-priori bound stands for: the float just below it, so that a power-of-two bound (|h| <= 1) maps
// [0, bound] into (-2^15, 2^15] — 2^15 itself is an fp16 number — instead of giving a bit of range away; 0: no bound
static unsigned bound_bits(float bound) {
  if (!(bound > 0.f)) return 0u;
  unsigned b;
  memcpy(&b, &bound, 4);
  return b > 0x00800000u ? b - 1 : b;
}
// one entry point for the bf16-plane and the scaled-fp16-plane packs (amax: the row maxima of planes = 2)
static int pk_pack_any(int planes, int transposed, const float *src, long long ld, int R, int C, void *dst, int rows_pad,
                       int row_off, int kb_off, int fill_rows, int fill_kb, int period, int shift, const uint32_t *amax,
                       nabu_stream_t stream) {
  if (planes == 2)
    return nabu_pk_pack_f16(transposed, src, ld, R, C, dst, rows_pad, row_off, kb_off, fill_rows, fill_kb, period, shift,
                            amax, stream);
  return nabu_pk_pack(planes, transposed, src, ld, R, C, dst, rows_pad, row_off, kb_off, fill_rows, fill_kb, period, shift,
                      stream);
}
static nabu_pk_gemm_desc pk_desc(int planes, int M, int N, int nkb, const void *A, int a_rows_pad, const void *B,
                                 int b_rows_pad, float *C, int ldc) {
  nabu_pk_gemm_desc g = {};
  g.size = sizeof(g); g.planes = planes; g.M = M; g.N = N; g.nkb = nkb; g.nbatch = 1;
  g.A[0] = A; g.B[0] = B; g.a_rows_pad = a_rows_pad; g.b_rows_pad = b_rows_pad; g.a_planes = g.b_planes = planes;
  g.C[0] = C; g.ldc = ldc; g.alpha = 1.f; g.beta = 0.f;
  if (planes == 2) g.a_amax[0] = g.a_amax[1] = g.b_amax[0] = g.b_amax[1] = reinterpret_cast<const uint32_t *>(16);   // sizing calls
  return g;
}

static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// workspace of the plain-arithmetic dense products of a layer
static size_t dense_ws_bytes(size_t B, size_t T, size_t D, size_t H) {
  const int M = (int)(B * T);
  size_t g = 0;
  g = max_sz(g, nabu_gemm_ws_bytes(M, (int)(4 * H), (int)D));            // x·Wx
  g = max_sz(g, nabu_gemm_ws_bytes(M, (int)D, (int)(4 * H)));            // dz·Wx^T
  g = max_sz(g, nabu_gemm_ws_bytes((int)D, (int)(4 * H), M));            // x^T·dz
  if (T > 1) g = max_sz(g, nabu_gemm_ws_bytes((int)H, (int)(4 * H), (int)(B * (T - 1))));
  return g;
}

// THE LAYER-NORMALISED CELL'S PATH through the driver, stated once: plain products (no packed planes), no companions,
// no persistent plan (the recurrence is the stepwise family of lstm_ln.hip), no profile events and no phase hook —
// every field of those stays 0 — and its own reserve and workspace carve.  (No bias: nabu_blstm_ln_* pass none.)
static Layout ln_layout(const nabu_blstm_desc *d) {
  Layout L = {};
  const size_t B = d->B, T = d->T, D = d->D, H = d->H;
  L.ln = true;
  L.out_stack = 1;
  L.fwd_only = (d->flags & NABU_BLSTM_FWD_ONLY) != 0;
  L.gates_elems = B * T * 4 * H;
  L.cs_elems = L.fwd_only ? 0 : B * T * H;
  L.rstd_elems = L.fwd_only ? 0 : B * T * 4;
  L.rstdc_elems = L.fwd_only ? 0 : B * T;
  L.reserve_bytes = 2 * (L.gates_elems + L.cs_elems + L.rstd_elems + L.rstdc_elems) * sizeof(float);
  size_t off = 0;
  const size_t st = align_up(2 * B * H * sizeof(float), 256);
  L.hstate_bytes = 2 * B * H * sizeof(float);
  L.hstate_off = off; off += st;
  L.cstate_off = off; off += st;
  L.dh_off = off; off += st;
  L.part_bytes = 20 * B * H * sizeof(float);
  L.part_off = off; off += align_up(L.part_bytes, 256);
  L.gemm_off = off; L.gemm_bytes = align_up(dense_ws_bytes(B, T, D, H), 256); off += L.gemm_bytes;
  L.total = off;
  return L;
}

static Layout make_layout(const nabu_blstm_desc *d, bool ln) {
  if (ln) return ln_layout(d);
  Layout L = {};
  L.hooks = true;
  const size_t B = d->B, T = d->T, D = d->D, H = d->H;
  L.gates_elems = B * T * 4 * H;
  L.cs_elems = B * T * H;
  L.reserve_bytes = (2 * L.gates_elems + 2 * L.cs_elems) * sizeof(float);
  L.res_dzT_off = L.res_dzT_bytes = 0;
  L.res_adzT_off = L.res_axT_off = L.res_aw2_off = L.res_ahT_off = L.res_xT_off = 0;
  L.pk_rowmax = L.pk_rowmax_bytes = 0;
  L.fwd_only = (d->flags & NABU_BLSTM_FWD_ONLY) != 0;
  size_t off = 2048;  // ws[0..4): persistent kernels' status word (0 = ok), zeroed by the caller once;
                      // ws[64..64+4*grid): XCC id of every block of the last forward launch (diagnostic)
  L.hstate_off = off; off += align_up(4 * B * H * sizeof(float), 256);
  L.cstate_off = off; off += align_up(2 * B * H * sizeof(float), 256);
  L.hstate_bytes = 4 * B * H * sizeof(float);
  const int M = (int)(B * T);
  const size_t g = max_sz(dense_ws_bytes(B, T, D, H), nabu_colsum_ws_bytes(M, (int)(4 * H)));
  L.gemm_off = off; L.gemm_bytes = align_up(g, 256); off += L.gemm_bytes;
  L.plan = plan_of(d);
  L.persist_bytes = align_up(L.plan.ws_bytes, 256);
  L.persist_off = off; off += L.persist_bytes;
  // narrow input projected inside the forward kernel (lstm_persist.h): its plane copy of x
  L.xws_bytes = align_up(L.plan.xws_bytes, 256);
  L.xws_off = off; off += L.xws_bytes;
  L.pk_planes = pk_planes_of(d);
  L.pk_in = L.pk_planes && D >= 256 && D % 4 == 0;
  L.pk_rec = L.pk_planes && T > 1;
  L.pk_whole = L.pk_rec && !L.pk_in && D % 4 == 0;
  L.pk_xw = L.pk_in || (L.pk_planes == 1 && D % 4 == 0);
  L.pk_off = off; L.pk_bytes = 0;
  if (L.pk_planes) {
    const int P = L.pk_planes, BT = (int)(B * T), G = (int)(4 * H);
    size_t fwd = 0, bwd = 0;
    auto take = [](size_t &o, size_t bytes) { const size_t at = o; o += align_up(bytes, 256); return at; };
    if (L.pk_xw) { L.pk_x = take(fwd, nabu_pk_bytes(BT, (int)D, P)); L.pk_w = take(fwd, nabu_pk_bytes(2 * G, (int)D, P)); }
    if (!L.fwd_only) {
      L.res_dzT_off = align_up(L.reserve_bytes, 256);
      L.res_dzT_bytes = nabu_pk_bytes(2 * G, BT, P);
      L.reserve_bytes = L.res_dzT_off + L.res_dzT_bytes;
      if (L.pk_in) {
        L.res_xT_off = align_up(L.reserve_bytes, 256);
        L.reserve_bytes = L.res_xT_off + nabu_pk_bytes((int)D, BT, P);
      }
    }
    L.pk_abwd_bytes = 0;
    if (P == 2) {
      const size_t aBT = 4 * (size_t)nabu_pk_rows_pad(BT), aG = 4 * (size_t)nabu_pk_rows_pad(2 * G), aD = 4 * (size_t)nabu_pk_rows_pad((int)D);
      const size_t aW = 4 * (size_t)nabu_pk_rows_pad((int)(L.pk_whole ? D + H : H));
      if (!L.fwd_only) {
        L.res_adzT_off = align_up(L.reserve_bytes, 256);
        L.res_axT_off = L.res_adzT_off + aG;
        L.res_aw2_off = L.res_axT_off + aD;
        L.reserve_bytes = L.res_aw2_off + aD;
        if (L.pk_in && L.pk_rec) {     // (not the whole-kernel form: its leading rows are measured maxima of x)
          L.res_ahT_off = L.reserve_bytes;
          L.reserve_bytes += aW;
        }
      }
      // (NABU_PK_AMAX_ATOMIC=1, the A/B switch of the maxima kernels, also has the backward pass measure again)
      static const int measure_twice = env_int("NABU_PK_AMAX_ATOMIC", 0);
      L.x_colmax_kept = !measure_twice && !L.fwd_only && L.pk_whole;
      L.pk_ax = take(fwd, aBT); L.pk_aw = take(fwd, aG);
      L.pk_adz = take(bwd, aBT);
      L.pk_ahT[0] = take(bwd, aW); L.pk_ahT[1] = take(bwd, aW);
      L.pk_abwd_bytes = bwd;
      if (L.pk_in && (size_t)2 * (H / 16) * BT * 4 < 0x80000000ull) {
        L.pk_rowmax_bytes = (size_t)2 * (H / 16) * BT * 4;
        L.pk_rowmax = take(bwd, L.pk_rowmax_bytes);
      }
    }
    if (L.pk_in) L.pk_xT = take(bwd, nabu_pk_bytes((int)D, BT, P));
    for (int dir = 0; dir < 2; ++dir)
      L.pk_hT[dir] = take(bwd, L.pk_rec ? nabu_pk_bytes((int)(L.pk_whole ? D + H : H), BT, P) : 0);
    if (L.pk_in) { L.pk_dz = take(bwd, nabu_pk_bytes(BT, 2 * G, P)); L.pk_w2 = take(bwd, nabu_pk_bytes((int)D, 2 * G, P)); }
    L.pk_bytes = max_sz(fwd, bwd);
    off += L.pk_bytes;
    // split-K slabs of the four products
    size_t gws = 0;
    nabu_pk_gemm_desc g;
    const int rpBT = nabu_pk_rows_pad(BT), rpG = nabu_pk_rows_pad(2 * G), rpD = nabu_pk_rows_pad((int)D);
    float *dummy = reinterpret_cast<float *>(16);
    if (L.pk_xw) {
      g = pk_desc(P, BT, 2 * G, nabu_pk_kblocks((int)D, P), dummy, rpBT, dummy, rpG, dummy, G); g.n_split = G; g.C2[0] = dummy;
      gws = max_sz(gws, nabu_gemm_pk_ws_bytes(&g));
    }
    if (L.pk_in) {
      g = pk_desc(P, (int)D, 2 * G, nabu_pk_kblocks(BT, P), dummy, rpD, dummy, rpG, dummy, G); g.n_split = G; g.C2[0] = dummy;
      gws = max_sz(gws, nabu_gemm_pk_ws_bytes(&g));
      g = pk_desc(P, BT, (int)D, nabu_pk_kblocks(2 * G, P), dummy, rpBT, dummy, rpD, dummy, (int)D);
      gws = max_sz(gws, nabu_gemm_pk_ws_bytes(&g));
    }
    if (L.pk_rec) {
      const int Mw = (int)(L.pk_whole ? D + H : H);
      g = pk_desc(P, Mw, G, nabu_pk_kblocks(BT, P), dummy, nabu_pk_rows_pad(Mw), dummy, rpG, dummy, G); g.nbatch = 2;
      g.A[1] = g.B[1] = dummy; g.C[1] = dummy;
      gws = max_sz(gws, nabu_gemm_pk_ws_bytes(&g));
    }
    if (gws > L.gemm_bytes) {   // the gemm region precedes the persist region: grow it in place
      const size_t grow = align_up(gws, 256) - L.gemm_bytes;
      L.gemm_bytes += grow; L.persist_off += grow; L.xws_off += grow; L.pk_off += grow; off += grow;
    }
  }
  // packed companions (ABI version 3)
  {
    const int BT = (int)(B * T), S = d->out_stack > 0 ? d->out_stack : 1;
    const bool P2 = L.pk_planes == 2;
    const int Mw = (int)(L.pk_whole ? D + H : H);
    L.out_stack = S;
    L.cmp_bytes[0] = (P2 && L.pk_in) ? nabu_pk_bytes(BT, (int)D, 2) : 0;
    L.cmp_bytes[1] = (P2 && L.pk_in) ? nabu_pk_bytes((int)D, BT, 2) : 0;
    L.cmp_bytes[2] = (P2 && L.pk_rec) ? 2 * nabu_pk_bytes(Mw, BT, 2) : 0;
    L.cmp_bytes[3] = (T % S == 0 && BT / S >= 1) ? nabu_pk_bytes(BT / S, (int)(2 * H) * S, 2) : 0;
    L.cmp_bytes[4] = (T % S == 0 && BT / S >= 1) ? nabu_pk_bytes((int)(2 * H) * S, BT / S, 2) : 0;
    L.x_pk = d->x_pk_rows != nullptr && L.cmp_bytes[0] != 0 && (L.fwd_only || d->x_pk_cols != nullptr);
    L.hT_ext = d->hT_pk != nullptr && L.cmp_bytes[2] != 0 && !L.fwd_only;
    size_t rows = nabu_pk_rows_pad(BT);
    rows = max_sz(rows, nabu_pk_rows_pad((int)(4 * H)));
    rows = max_sz(rows, nabu_pk_rows_pad((int)(D + H)));
    L.cmp_amax_bytes = align_up(4 * rows, 256);
    L.cmp_amax_off = off; off += L.cmp_amax_bytes;
  }
  L.total = off;
  return L;
}

// the row "maximum" of a packed companion: |h| <= 1 at the scale 2^14 the recurrent kernel splits its planes at
static constexpr unsigned CMP_AMAX_BITS = 0x3F800000u;

// optional profiling hook: caller-owned events recorded around the recurrent kernels
static thread_local hipEvent_t g_ev_begin = nullptr, g_ev_end = nullptr;
// optional hook between the recurrent kernel(s) and the dense products of nabu_blstm_bwd
static thread_local nabu_phase_hook_t g_phase_hook = nullptr;
static thread_local void *g_phase_user = nullptr;

static bool use_persistent(const nabu_blstm_desc *d, const PersistPlan &plan) {
  return d->mode != NABU_LSTM_STEPWISE && plan.supported;
}

// WHAT A RESERVE HOLDS is decided by make_layout from the descriptor AND from process state (the default GEMM
// precision, NABU_PK, the device's LDS class): the forward call records a fingerprint of the layout it wrote, keyed by
// the reserve's address, and the backward calls compare it with the layout THEY derive before they touch the buffer —
// a reserve that no forward call produced, or one produced under another layout (precision switched in between, a
// forward-only descriptor), is rejected with NABU_EINVAL instead of being read as something it is not.  Host memory
// only: no device round trip, and the check works (and is tested) without a GPU.
struct ReserveTag {
  const void *reserve;
  uint64_t serial;
  int32_t B, T, D, H, planes, flags, rec;
  uint8_t pk_in, pk_rec, pk_whole;
  size_t reserve_bytes, res_dzT_off;
};
static ReserveTag tag_of(const nabu_blstm_desc *d, const Layout &L, const void *reserve) {
  ReserveTag t = {};
  t.reserve = reserve; t.B = d->B; t.T = d->T; t.D = d->D; t.H = d->H; t.planes = L.pk_planes; t.flags = d->flags;
  t.rec = d->recurrent_precision;
  t.pk_in = L.pk_in; t.pk_rec = L.pk_rec; t.pk_whole = L.pk_whole;
  t.reserve_bytes = L.reserve_bytes; t.res_dzT_off = L.res_dzT_off;
  return t;
}
// one table per family of entry points: the least recently written tag is replaced (a reserve whose tag fell out is
// rejected, see nabu_hip.h), and a reserve of the other family's forward call is "not written" by this one's
struct TagTable {
  const char *writer;
  ReserveTag *tags;
  int n;
  std::mutex mutex;
  uint64_t serial;
  void store(const ReserveTag &t) {
    std::lock_guard<std::mutex> lock(mutex);
    ReserveTag *slot = &tags[0];
    for (ReserveTag *e = tags; e < tags + n; ++e) {
      if (e->reserve == t.reserve) { slot = e; break; }
      if (e->serial < slot->serial) slot = e;          // least recently written
    }
    *slot = t;
    slot->serial = ++serial;
  }
  int check(const ReserveTag &want, const char *who) {
    std::lock_guard<std::mutex> lock(mutex);
    for (const ReserveTag *it = tags; it < tags + n; ++it) {
      const ReserveTag &e = *it;
      if (e.reserve != want.reserve || !e.serial) continue;
      if (e.B == want.B && e.T == want.T && e.D == want.D && e.H == want.H && e.planes == want.planes && e.flags == want.flags &&
          e.rec == want.rec && e.pk_in == want.pk_in && e.pk_rec == want.pk_rec && e.pk_whole == want.pk_whole &&
          e.reserve_bytes == want.reserve_bytes && e.res_dzT_off == want.res_dzT_off)
        return 0;
      return fail(NABU_EINVAL, "%s: the reserve was written by %s under another layout (B %d T %d D %d H %d, %d planes, "
                  "%zu bytes, flags %d; this call: B %d T %d D %d H %d, %d planes, %zu bytes) — descriptor or process precision "
                  "changed between the passes", who, writer, e.B, e.T, e.D, e.H, e.planes, e.reserve_bytes, e.flags, want.B,
                  want.T, want.D, want.H, want.planes, want.reserve_bytes);
    }
    return fail(NABU_EINVAL, "%s: no %s call of this process wrote this reserve (%p)", who, writer, want.reserve);
  }
};
static ReserveTag g_tag_slots[4096], g_ln_tag_slots[1024];
static TagTable g_tags = {"nabu_blstm_fwd", g_tag_slots, 4096}, g_ln_tags = {"nabu_blstm_ln_fwd", g_ln_tag_slots, 1024};
static TagTable &tags_of(const Layout &L) { return L.ln ? g_ln_tags : g_tags; }
static void tag_store(const nabu_blstm_desc *d, const Layout &L, const void *reserve) { tags_of(L).store(tag_of(d, L, reserve)); }
static int tag_check(const nabu_blstm_desc *d, const Layout &L, const void *reserve, const char *who) {
  if (L.fwd_only) return fail(NABU_EINVAL, "%s: the descriptor says NABU_BLSTM_FWD_ONLY — its reserve has no room for a backward pass", who);
  const ReserveTag want = tag_of(d, L, reserve);
  return tags_of(L).check(want, who);
}

// ---------------------------------------------------------------------------
// THE CELL'S OWN ARGUMENTS of a layer call: bias and bias gradients (plain), or gamma / beta and their gradients (ln; null
// in nabu_blstm_ln_bwd_weights, which reads none of them).  WHICH cell a call runs is said once, by the entry point's
// DescScope, and kept in Layout::ln.
struct Cell {
  const nabu_blstm_ln_params *ln;
  const float *bias[2];
  float *dbias[2];
};
static Cell plain_cell(const float *bias_fw, const float *bias_bw, float *dbias_fw, float *dbias_bw) {
  return Cell{nullptr, {bias_fw, bias_bw}, {dbias_fw, dbias_bw}};
}
static Cell ln_cell(const nabu_blstm_ln_params *ln) { return Cell{ln, {nullptr, nullptr}, {nullptr, nullptr}}; }

// grads = a call that writes the bias resp. gamma / beta gradients
static int check_cell(const Layout &L, const Cell &cell, bool grads, const char *who) {
  if (!L.ln) {
    NABU_CHECK_ARG(grads ? cell.dbias[0] && cell.dbias[1] : cell.bias[0] && cell.bias[1], "%s: null pointer", who);
    return 0;
  }
  const nabu_blstm_ln_params *ln = cell.ln;
  if (!ln || ln->size != sizeof(nabu_blstm_ln_params)) return fail(NABU_EINVAL, "%s: bad nabu_blstm_ln_params size", who);
  for (int dir = 0; dir < 2; ++dir)
    for (int k = 0; k < 5; ++k) {
      if (!ln->gamma[dir][k] || !ln->beta[dir][k]) return fail(NABU_EINVAL, "%s: null gamma/beta pointer", who);
      if (grads && (!ln->dgamma[dir][k] || !ln->dbeta[dir][k])) return fail(NABU_EINVAL, "%s: null dgamma/dbeta pointer", who);
    }
  return 0;
}

// one layer call as its stages see it
struct Call {
  const nabu_blstm_desc *d;
  const Layout &L;
  const Cell &cell;
  int B, T, D, H, max_len;
  const float *x;
  const int32_t *len;
  const float *kern[2];
  float *gates[2], *cs[2];
  char *reserve, *w;       // the reserve and the workspace, as bytes
  nabu_stream_t stream;
  hipStream_t s;
  float *out;              // forward
  const float *h, *d_out;  // backward: the forward call's out, its gradient
  float *d_x, *dkern[2];

  Call(const nabu_blstm_desc *d_, const Layout &L_, const Cell &cell_, const float *x_, const int32_t *len_,
       const float *kernel_fw, const float *kernel_bw, void *reserve_, void *ws, nabu_stream_t stream_)
      : d(d_), L(L_), cell(cell_), B(d_->B), T(d_->T), D(d_->D), H(d_->H), max_len(d_->max_len > 0 ? d_->max_len : d_->T),
        x(x_), len(len_), kern{kernel_fw, kernel_bw}, reserve(static_cast<char *>(reserve_)), w(static_cast<char *>(ws)),
        stream(stream_), s(static_cast<hipStream_t>(stream_)), out(nullptr), h(nullptr), d_out(nullptr), d_x(nullptr),
        dkern{nullptr, nullptr} {
    float *r = static_cast<float *>(reserve_);
    gates[0] = r; gates[1] = r + L.gates_elems;
    cs[0] = r + 2 * L.gates_elems; cs[1] = cs[0] + L.cs_elems;
  }
  float *gemm_ws() const { return reinterpret_cast<float *>(w + L.gemm_off); }
  template <typename Tp> Tp *in_reserve(size_t off) const { return reinterpret_cast<Tp *>(reserve + off); }
  int mark(hipEvent_t ev) const {     // profile event
    if (L.hooks && ev) NABU_HIP(hipEventRecord(ev, s));
    return 0;
  }
};

// ---------------------------------------------------------------------------
// stage: rows [max_len, T) of a [B, T, width] tensor, which the recurrence never visits, are zero
static int zero_unvisited_frames(const Call &c, float *base, size_t width) {
  if (c.max_len < c.T)
    NABU_HIP(hipMemset2DAsync(base + (size_t)c.max_len * width, (size_t)c.T * width * sizeof(float), 0,
                              (size_t)(c.T - c.max_len) * width * sizeof(float), c.B, c.s));
  return 0;
}

// stage: the time-batched input projections gates_d = x·Wx_d (+ b_d), on row-major operands
static int project_input_plain(const Call &c) {
  for (int dir = 0; dir < 2; ++dir)
    NABU_TRY(nabu_gemm_ex(c.d->gemm_precision, 0, 0, c.B * c.T, 4 * c.H, c.D, 1.f, c.x, c.D, c.kern[dir], 4 * c.H, 0.f,
                          c.gates[dir], 4 * c.H, c.cell.bias[dir], 0, 0, 0, c.gemm_ws(), c.L.gemm_bytes, c.stream));
  return 0;
}

// ... on packed bf16-plane operands: X once, Wx^T of both cells as the rows of ONE operand; one product fills the gate
// buffers of both directions.  clear_ring: the fill launch also clears the persistent launch's exchange ring
// (PersistPlan::caller_ring_words); *ring_cleared says whether it did
static int project_input_packed(const Call &c, bool clear_ring, bool *ring_cleared) {
  const Layout &L = c.L;
  const nabu_blstm_desc *d = c.d;
  const int B = c.B, T = c.T, D = c.D, H = c.H;
  const float *x = c.x;
  hipStream_t s = c.s;
  const int P = L.pk_planes, BT = B * T, G = 4 * H;
  char *pk = c.w + L.pk_off;
  const int rpBT = nabu_pk_rows_pad(BT), rpG = nabu_pk_rows_pad(2 * G), nkb = nabu_pk_kblocks(D, P);
  uint32_t *ax = reinterpret_cast<uint32_t *>(pk + L.pk_ax), *aw = reinterpret_cast<uint32_t *>(pk + L.pk_aw);
  if (P == 2) {
    // f16x3: the frames' and the gate columns' largest magnitudes first.  The input: from the caller's bound where
    // one is given (x_bound: the previous layer's LSTM outputs — no pass over x), measured otherwise (the features).
    // The maxima the BACKWARD pass needs of the same tensors (columns of x, rows of Wx) come out of the same reads
    // and wait in the reserve — unless no backward pass follows.
    uint32_t *axT = L.fwd_only ? nullptr : c.in_reserve<uint32_t>(L.res_axT_off);
    uint32_t *aw2 = L.fwd_only ? nullptr : c.in_reserve<uint32_t>(L.res_aw2_off);
    const unsigned xb = L.x_pk ? CMP_AMAX_BITS : bound_bits(d->x_bound);     // (a packed companion: scale 2^14)
    const int rpD = nabu_pk_rows_pad(D);
    // (and the backward pass's row bound of h^T, |h| <= 1: a constant it would otherwise fill in a launch of its own)
    uint32_t *ahT = L.res_ahT_off ? c.in_reserve<uint32_t>(L.res_ahT_off) : nullptr;
    // and the recurrent launch's exchange ring (lstm_persist.h: caller_ring_words) — nothing between here and that
    // launch writes the persistent kernels' part of the workspace
    FillSeg fill[6] = {{ax, (size_t)rpBT, xb}, {aw, (size_t)rpG, 0u}, {axT, axT ? (size_t)rpD : 0, xb}, {aw2, aw2 ? (size_t)rpD : 0, 0u},
                       {ahT, ahT ? (size_t)nabu_pk_rows_pad(H) : 0, L.hT_ext ? CMP_AMAX_BITS : bound_bits(1.0f)},
                       {c.w + L.persist_off, clear_ring ? L.plan.caller_ring_words : 0, 0xFFFFFFFFu}};
    NABU_TRY(multi_fill(fill, 6, s));
    *ring_cleared = fill[5].words > 0;
    if (!xb) NABU_TRY(nabu_pk_amax(x, D, BT, D, ax, axT, c.stream));
    NABU_TRY(pk_amax_pair(c.kern[0], c.kern[1], G, D, G, aw2, aw, aw + G, nullptr, s));
  }
  // the input operand: the producer layer's forward kernel wrote it (x_pk_rows) — or one pass over x here
  const void *xop = L.x_pk ? d->x_pk_rows : pk + L.pk_x;
  if (!L.x_pk && L.res_xT_off) {
    // ... and x^T for the backward pass's weight-gradient product out of the same read (kept in the reserve)
    const int rpDx = nabu_pk_rows_pad(D);
    NABU_TRY(pk_pack_both(P, x, D, BT, D, pk + L.pk_x, rpBT, 0, rpBT, nkb, c.reserve + L.res_xT_off, rpDx, 0, rpDx,
                          nabu_pk_kblocks(BT, P), s, P == 2 ? ax : nullptr,
                          P == 2 ? c.in_reserve<uint32_t>(L.res_axT_off) : nullptr));
  } else if (!L.x_pk) {
    NABU_TRY(pk_pack_any(P, 0, x, D, BT, D, pk + L.pk_x, rpBT, 0, 0, rpBT, nkb, 0, 0, ax, c.stream));
  }
  {   // Wx^T of both cells: one launch
    PkPackReq rq[2];
    for (int dir = 0; dir < 2; ++dir)
      rq[dir] = PkPackReq{c.kern[dir], G, D, G, pk + L.pk_w, rpG, dir * G, 0, dir ? rpG - G : G, nkb, 0, 0, P == 2 ? aw : nullptr};
    NABU_TRY(pk_pack_multi(P, 1, rq, 2, s));
  }
  nabu_pk_gemm_desc g = pk_desc(P, BT, 2 * G, nkb, xop, rpBT, pk + L.pk_w, rpG, c.gates[0], G);
  g.C2[0] = c.gates[1]; g.n_split = G; g.bias = c.cell.bias[0]; g.bias2 = c.cell.bias[1];
  if (P == 2) { g.a_amax[0] = ax; g.b_amax[0] = aw; g.direct = 2; }
  return nabu_gemm_pk(&g, c.w + L.gemm_off, L.gemm_bytes, c.stream);
}

static int project_input(const Call &c, bool clear_ring, bool *ring_cleared) {
  return c.L.pk_xw ? project_input_packed(c, clear_ring, ring_cleared) : project_input_plain(c);
}

// ---------------------------------------------------------------------------
// stage: packed companions of the output (ABI version 3): out of the recurrent kernel itself where that is possible, by
// the pack kernels behind the recurrence otherwise — complete on return either way
static bool wants_companions(const nabu_blstm_desc *d, const Layout &L) {
  return ((d->out_pk_rows || d->out_pk_cols) && L.cmp_bytes[3] != 0) || L.hT_ext;
}
static bool kernel_emits(const nabu_blstm_desc *d, const Layout &L) {
  if (!wants_companions(d, L) || !use_persistent(d, L.plan) || !L.plan.emits) return false;
  for (int i = 2; i < 5; ++i)
    if (L.cmp_bytes[i] >= 0x7FFFFFF0ull) return false;      // 32-bit buffer offsets inside the kernel
  return true;
}
// which companions the recurrent kernel writes itself: bit 0 rows, bit 1 transposed, bit 2 h^T.  Default 4: measured on
// cfg2, the 2-byte stores of the transposed operand and the extra live state of the rows cost the forward kernel what the
// pack kernels they replace cost; NABU_PERSIST_EMIT_MASK=7 writes all three from the kernel, 0 none
// (... and not from the launch that also projects its input (the first layer, XIN): there the h^T stores cost 0.09 ms
// per cfg2 step against 0.05 for the pack they replace — per-launch events, LABNOTES.md section 9.  The switch, when set,
// is taken literally.)
static int emit_mask_env(bool *from_env = nullptr) {
  static int m = -1;
  static bool set = false;
  if (m < 0) { const char *e = getenv("NABU_PERSIST_EMIT_MASK"); set = e != nullptr; m = e ? (atoi(e) & 7) : 4; }
  if (from_env) *from_env = set;
  return m;
}
static int emitted_by_kernel(const nabu_blstm_desc *d, const Layout &L) {
  if (!kernel_emits(d, L)) return 0;
  bool from_env = false;
  int m = emit_mask_env(&from_env);
  if (!from_env && L.plan.fuses_input) m &= ~4;
  const bool want_out = (d->out_pk_rows || d->out_pk_cols) && L.cmp_bytes[3] != 0;
  if (!want_out || !d->out_pk_rows) m &= ~1;
  if (!want_out || !d->out_pk_cols) m &= ~2;
  if (!L.hT_ext) m &= ~4;
  return m;
}
// which companions this call owes, who writes them and where
struct Companions {
  bool wanted;
  bool want_out;
  int by_kernel;      // bits written by the recurrent kernel itself (emitted_by_kernel)
  int S, rpW, r0;
  char *hTp[2];
  EmitArgs em;
};
static Companions plan_companions(const Call &c) {
  const Layout &L = c.L;
  const nabu_blstm_desc *d = c.d;
  Companions m = {};
  m.wanted = wants_companions(d, L);
  m.S = L.out_stack; m.rpW = nabu_pk_rows_pad(L.pk_whole ? c.D + c.H : c.H); m.r0 = L.pk_whole ? c.D : 0;
  if (L.hT_ext) { m.hTp[0] = static_cast<char *>(d->hT_pk); m.hTp[1] = m.hTp[0] + L.cmp_bytes[2] / 2; }
  m.want_out = (d->out_pk_rows || d->out_pk_cols) && L.cmp_bytes[3] != 0;
  m.by_kernel = emitted_by_kernel(d, L);
  if (m.by_kernel) {
    EmitArgs &em = m.em;
    em.x_rows = (m.want_out && (m.by_kernel & 1)) ? static_cast<char *>(d->out_pk_rows) : nullptr;
    em.x_cols = (m.want_out && (m.by_kernel & 2)) ? static_cast<char *>(d->out_pk_cols) : nullptr;
    em.hT[0] = (m.by_kernel & 4) ? m.hTp[0] : nullptr; em.hT[1] = (m.by_kernel & 4) ? m.hTp[1] : nullptr;
    em.x_rows_pad = (unsigned)nabu_pk_rows_pad(c.B * c.T / m.S);
    em.x_cols_pad = (unsigned)nabu_pk_rows_pad(2 * c.H * m.S);
    em.hT_rows_pad = (unsigned)m.rpW;
    em.hT_row0 = m.r0;
    em.stack_shift = m.S == 2 ? 1 : 0;
    em.b0 = 0;
  }
  return m;
}
// todo: the bits (0 rows, 1 transposed, 2 h^T) the recurrent kernel did not write
static int companions_by_pack_kernels(const Call &c, const Companions &m, int todo) {
  const Layout &L = c.L;
  const nabu_blstm_desc *d = c.d;
  const int B = c.B, T = c.T, H = c.H, S = m.S;
  if (!m.wanted) return 0;
  todo &= ((m.want_out && d->out_pk_rows) ? 1 : 0) | ((m.want_out && d->out_pk_cols) ? 2 : 0) | (L.hT_ext ? 4 : 0);
  if (!todo) return 0;
  uint32_t *am = reinterpret_cast<uint32_t *>(c.w + L.cmp_amax_off);
  const FillSeg fill = {am, L.cmp_amax_bytes / 4, CMP_AMAX_BITS};
  NABU_TRY(multi_fill(&fill, 1, c.s));
  const int R = B * T / S, C = 2 * H * S;
  if (todo & 1)
    NABU_TRY(pk_pack_any(2, 0, c.out, C, R, C, d->out_pk_rows, nabu_pk_rows_pad(R), 0, 0, nabu_pk_rows_pad(R), nabu_pk_kblocks(C, 2), 0, 0, am, c.stream));
  if (todo & 2)
    NABU_TRY(pk_pack_any(2, 1, c.out, C, R, C, d->out_pk_cols, nabu_pk_rows_pad(C), 0, 0, nabu_pk_rows_pad(C), nabu_pk_kblocks(R, 2), 0, 0, am, c.stream));
  if (todo & 4) {
    PkPackReq rq[2];
    for (int dir = 0; dir < 2; ++dir)
      rq[dir] = PkPackReq{c.out + (size_t)dir * H, 2 * H, B * T, H, m.hTp[dir], m.rpW, m.r0, 0, m.rpW - m.r0, nabu_pk_kblocks(B * T, 2), T, dir ? 1 : -1, am};
    NABU_TRY(pk_pack_multi(2, 1, rq, 2, c.s));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// stage: the stepwise recurrence, one (plain) resp. two (layer norm) launches per timestep over zeroed states
static LnArgs ln_args(const Call &c) {
  const Layout &L = c.L;
  LnArgs p = {};
  p.B = c.B; p.T = c.T; p.D = c.D; p.H = c.H; p.max_len = c.max_len;
  p.save = L.fwd_only ? 0 : 1;
  p.len = c.len;
  for (int dir = 0; dir < 2; ++dir) { p.kernel[dir] = c.kern[dir]; p.gates[dir] = c.gates[dir]; p.cs[dir] = c.cs[dir]; }
  p.rstd[0] = c.cs[1] + L.cs_elems; p.rstd[1] = p.rstd[0] + L.rstd_elems;
  p.rstdc[0] = p.rstd[1] + L.rstd_elems; p.rstdc[1] = p.rstdc[0] + L.rstdc_elems;
  if (c.cell.ln)
    for (int dir = 0; dir < 2; ++dir)
      for (int k = 0; k < 5; ++k) { p.gamma[dir][k] = c.cell.ln->gamma[dir][k]; p.beta[dir][k] = c.cell.ln->beta[dir][k]; }
  p.out = c.out; p.dout = c.d_out;
  p.hstate = reinterpret_cast<float *>(c.w + L.hstate_off);
  p.cstate = reinterpret_cast<float *>(c.w + L.cstate_off);
  p.dh = reinterpret_cast<float *>(c.w + L.dh_off);
  p.part = reinterpret_cast<float *>(c.w + L.part_off);
  return p;
}
static StepArgs step_args(const Call &c) {
  StepArgs p;
  p.B = c.B; p.T = c.T; p.D = c.D; p.H = c.H; p.max_len = c.max_len; p.len = c.len;
  for (int i = 0; i < 2; ++i) { p.kernel[i] = c.kern[i]; p.gates[i] = c.gates[i]; p.cs[i] = c.cs[i]; }
  p.out = c.out; p.dout = c.d_out;
  p.hstate = reinterpret_cast<float *>(c.w + c.L.hstate_off);
  p.cstate = reinterpret_cast<float *>(c.w + c.L.cstate_off);
  return p;
}
static dim3 step_grid(const Call &c) { return dim3((c.H + SU - 1) / SU, (c.B + SB - 1) / SB, 2); }

static int stepwise_fwd(const Call &c) {
  const size_t state = 2 * (size_t)c.B * c.H * sizeof(float);
  NABU_HIP(hipMemsetAsync(c.w + c.L.hstate_off, 0, c.L.hstate_bytes, c.s));
  NABU_HIP(hipMemsetAsync(c.w + c.L.cstate_off, 0, state, c.s));
  if (c.L.ln) return ln_recurrence_fwd(ln_args(c), c.s);
  const StepArgs p = step_args(c);
  const size_t shm = ((size_t)SB * c.H + SB * 4 * SU) * sizeof(float);
  NABU_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(lstm_step_fwd_kernel), shm));
  NABU_TRY(c.mark(g_ev_begin));
  for (int t = 0; t < c.max_len; ++t) hipLaunchKernelGGL(lstm_step_fwd_kernel, step_grid(c), dim3(STEP_NT), shm, c.s, p, t);
  NABU_LAUNCH_CHECK();
  return c.mark(g_ev_end);
}

static int stepwise_bwd(const Call &c) {
  NABU_HIP(hipMemsetAsync(c.w + c.L.cstate_off, 0, 2 * (size_t)c.B * c.H * sizeof(float), c.s));   // the dc carry
  if (c.L.ln) {
    NABU_HIP(hipMemsetAsync(c.w + c.L.part_off, 0, c.L.part_bytes, c.s));
    return ln_recurrence_bwd(ln_args(c), c.s);
  }
  const StepArgs p = step_args(c);
  for (int t = c.max_len - 1; t >= 0; --t) hipLaunchKernelGGL(lstm_step_bwd_kernel, step_grid(c), dim3(STEP_NT), 0, c.s, p, t);
  NABU_LAUNCH_CHECK();
  return 0;
}

// stage: the forward recurrence and the companions behind it.  Persistent where the plan has a kernel for the shape;
// a grid that cannot be co-resident on this device (the occupancy check before the launch says NABU_EUNSUP) steps
// instead under NABU_LSTM_AUTO
// (x_colmax_kept, for a forward path whose launch did not measure them)
static int keep_x_colmax(const Call &c) {
  uint32_t *keep = c.in_reserve<uint32_t>(c.L.res_axT_off);
  const FillSeg fill = {keep, (size_t)c.D, 0u};
  NABU_TRY(multi_fill(&fill, 1, c.s));
  return nabu_pk_amax(c.x, c.D, c.B * c.T, c.D, nullptr, keep, c.stream);
}

static int recurrence_fwd(const Call &c, bool projected, bool ring_cleared) {
  const Layout &L = c.L;
  const Companions m = plan_companions(c);
  if (use_persistent(c.d, L.plan)) {
    const bool fuse_in = L.plan.fuses_input;
    NABU_TRY(c.mark(g_ev_begin));
    const int e = lstm_persist_fwd(L.plan, c.len, c.kern, c.gates, c.cs, c.out, reinterpret_cast<int *>(c.w), c.w + L.persist_off,
                                   L.persist_bytes, c.s, ring_cleared, fuse_in ? c.x : nullptr, fuse_in ? c.cell.bias : nullptr,
                                   L.xws_bytes ? c.w + L.xws_off : nullptr, m.by_kernel ? &m.em : nullptr,
                                   L.x_colmax_kept ? c.in_reserve<uint32_t>(L.res_axT_off) : nullptr);
    if (!(e == NABU_EUNSUP && c.d->mode == NABU_LSTM_AUTO)) {
      if (e) return e;
      NABU_TRY(c.mark(g_ev_end));
      // (the launch prepared x as planes, and measured it, exactly where it fused the input and has a plane copy)
      if (L.x_colmax_kept && !(fuse_in && L.plan.xws_bytes)) NABU_TRY(keep_x_colmax(c));
      return companions_by_pack_kernels(c, m, 7 & ~m.by_kernel);
    }
    if (!projected) {   // the step kernels read the projection from the gate buffers
      bool unused = false;
      NABU_TRY(project_input(c, false, &unused));
    }
  }
  NABU_TRY(stepwise_fwd(c));
  if (L.x_colmax_kept) NABU_TRY(keep_x_colmax(c));
  return companions_by_pack_kernels(c, m, 7);
}

static const char *const ENTRY[2][4] = {{"blstm_fwd", "blstm_bwd_data", "blstm_bwd_weights", "blstm_bwd"},
                                        {"blstm_ln_fwd", "blstm_ln_bwd_data", "blstm_ln_bwd_weights", "blstm_ln_bwd"}};

// THE FORWARD PASS of a layer, either cell
static int blstm_forward(const DescScope &scope, const Cell &cell, const float *x, const int32_t *len, const float *kernel_fw,
                         const float *kernel_bw, float *out, void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  if (scope.err) return scope.err;
  const nabu_blstm_desc *d = &scope.d;
  const char *who = ENTRY[scope.ln][0];
  const Layout L = make_layout(d, scope.ln);
  NABU_CHECK_ARG(x && len && kernel_fw && kernel_bw && out && reserve && ws, "%s: null pointer", who);
  NABU_TRY(check_cell(L, cell, false, who));
  if (ws_bytes < L.total) return fail(NABU_EWS, "%s: workspace %zu < %zu", who, ws_bytes, L.total);
  if (d->mode == NABU_LSTM_PERSISTENT && !L.plan.supported)
    return fail(NABU_EUNSUP, "%s: persistent kernel does not support B=%d H=%d", who, d->B, d->H);
  tag_store(d, L, reserve);
  Call c(d, L, cell, x, len, kernel_fw, kernel_bw, reserve, ws, stream);
  c.out = out;
  // narrow input (first layer): the persistent kernel projects its input itself (lstm_persist.hip, XK) — no product here
  const bool persistent = use_persistent(d, L.plan);
  const bool projected = !(persistent && L.plan.fuses_input);
  bool ring_cleared = false;
  if (projected) NABU_TRY(project_input(c, persistent, &ring_cleared));
  NABU_TRY(zero_unvisited_frames(c, out, 2 * (size_t)c.H));
  return recurrence_fwd(c, projected, ring_cleared);
}

// ---------------------------------------------------------------------------
// what the persistent backward kernels leave behind besides dz
struct PersistOut {
  float *db_part;     // bias-gradient partials [db_rows][2][4H]; null: the recurrence stepped
  int db_rows;
  bool db_done;       // the bias gradients were summed by the launch that read the maxima
  uint32_t *rowmax;   // f16x3 with an input gradient: every workgroup's row maxima of dz, asked for in the workspace
  bool rowmax_done;
};

// stage: the backward recurrence (dz in place over the activations), with the forward pass's fallback rule
static int recurrence_bwd(const Call &c, PersistOut *po) {
  const Layout &L = c.L;
  NABU_TRY(c.mark(g_ev_begin));
  bool stepwise = !use_persistent(c.d, L.plan);
  if (!stepwise) {
    const int e = lstm_persist_bwd(L.plan, c.len, c.kern, c.gates, c.cs, c.d_out, reinterpret_cast<int *>(c.w), c.w + L.persist_off,
                                   L.persist_bytes, &po->db_part, &po->db_rows, c.s, po->rowmax, &po->rowmax_done);
    if (e == NABU_EUNSUP && c.d->mode == NABU_LSTM_AUTO) { stepwise = true; po->db_part = nullptr; po->db_rows = 0; po->rowmax_done = false; }
    else if (e) return e;
  }
  if (stepwise) NABU_TRY(stepwise_bwd(c));
  NABU_TRY(c.mark(g_ev_end));
  if (L.hooks && g_phase_hook) g_phase_hook(g_phase_user);
  return 0;
}

// ---------------------------------------------------------------------------
// stages: the backward products on packed bf16-plane operands (gemm_pk.hip).  dZ^T of both cells is one operand
// [8H, BT] (in the reserve): the weight gradients of both cells are column ranges of one product (input part) resp. a
// batch of two (recurrent part)
struct PackedBwd {
  int P, G, M, rpBT, rpG, rpD, nkbT, nkb2, kbG;
  char *pk, *dzTp;
  // f16x3 (P = 2): row maxima of every operand — measured (dz, the weights, x) or known (|h| < 1)
  uint32_t *adz, *axT, *aw2, *ahT[2], *adzT;
  explicit PackedBwd(const Call &c) {
    const Layout &L = c.L;
    P = L.pk_planes; G = 4 * c.H; M = c.B * c.T;
    pk = c.w + L.pk_off;
    dzTp = c.reserve + L.res_dzT_off;
    rpBT = nabu_pk_rows_pad(M); rpG = nabu_pk_rows_pad(2 * G); rpD = nabu_pk_rows_pad(c.D);
    nkbT = nabu_pk_kblocks(M, P);
    nkb2 = nabu_pk_kblocks(2 * G, P); kbG = G / 16;
    adz = reinterpret_cast<uint32_t *>(pk + L.pk_adz);
    axT = c.in_reserve<uint32_t>(L.res_axT_off);    // from the forward pass
    aw2 = c.in_reserve<uint32_t>(L.res_aw2_off);
    ahT[0] = reinterpret_cast<uint32_t *>(pk + L.pk_ahT[0]); ahT[1] = reinterpret_cast<uint32_t *>(pk + L.pk_ahT[1]);
    adzT = c.in_reserve<uint32_t>(L.res_adzT_off);
  }
};

// data part: dz packed transposed (and row-major where dx follows: both packs from one read of dz)
static int pack_dz(const Call &c, const PackedBwd &k, PersistOut *po) {
  const Layout &L = c.L;
  const int P = k.P, G = k.G, M = k.M, H = c.H;
  const bool both = c.d_x && L.pk_in;
  if (P == 2) {
    // the maxima of dz: its rows' over BOTH cells (the row scale of dZ as [BT, 8H]) and its columns'
    if (po->db_part && (!both || po->rowmax_done)) {
      // the persistent kernel kept them: the gate columns' maxima per unit next to its bias-gradient partials, the
      // frames' per workgroup in the workspace (only asked for where an input gradient follows) — no read of dz
      // (the bias gradients — the sum of the same units' partial rows — come out of the same launch)
      NABU_TRY(pk_amax_from_persist(M, k.rpBT, c.T, c.max_len, 2 * (H / 16), po->rowmax, both ? k.adz : nullptr, po->db_rows,
                                    2 * G, po->db_part + lstm_persist_db_floats(c.B, H), 2 * G, k.adzT, c.s, po->db_part,
                                    c.cell.dbias[0], c.cell.dbias[1]));
      po->db_done = true;
    } else {
      const FillSeg fill[2] = {{k.adz, both ? (size_t)k.rpBT : 0, 0u}, {k.adzT, (size_t)k.rpG, 0u}};
      NABU_TRY(multi_fill(fill, 2, c.s));
      NABU_TRY(pk_amax_pair(c.gates[0], c.gates[1], G, M, G, both ? k.adz : nullptr, k.adzT, k.adzT + G, nullptr, c.s));
    }
  }
  for (int dir = 0; dir < 2; ++dir) {
    if (both)
      NABU_TRY(pk_pack_both(P, c.gates[dir], G, M, G, k.pk + L.pk_dz, k.rpBT, dir * k.kbG, k.rpBT, dir ? k.nkb2 - k.kbG : k.kbG,
                            k.dzTp, k.rpG, dir * G, dir ? k.rpG - G : G, k.nkbT, c.s, k.adz, k.adzT));
    else
      NABU_TRY(pk_pack_any(P, 1, c.gates[dir], G, M, G, k.dzTp, k.rpG, dir * G, 0, dir ? k.rpG - G : G, k.nkbT, 0, 0, k.adzT,
                           c.stream));
  }
  return 0;
}

// dx = [dZ_fw | dZ_bw] · [Wx_fw | Wx_bw]^T: the two cells are two ranges of ONE reduction
static int packed_dx(const Call &c, const PackedBwd &k) {
  const Layout &L = c.L;
  const int P = k.P, G = k.G, D = c.D;
  PkPackReq rq[2];
  for (int dir = 0; dir < 2; ++dir)
    rq[dir] = PkPackReq{c.kern[dir], G, D, G, k.pk + L.pk_w2, k.rpD, 0, dir * k.kbG, k.rpD, dir ? k.nkb2 - k.kbG : k.kbG, 0, 0,
                        P == 2 ? k.aw2 : nullptr};
  NABU_TRY(pk_pack_multi(P, 0, rq, 2, c.s));
  nabu_pk_gemm_desc g = pk_desc(P, k.M, D, k.nkb2, k.pk + L.pk_dz, k.rpBT, k.pk + L.pk_w2, k.rpD, c.d_x, D);
  if (P == 2) { g.a_amax[0] = k.adz; g.b_amax[0] = k.aw2; g.direct = 2; }
  return nabu_gemm_pk(&g, c.w + L.gemm_off, L.gemm_bytes, c.stream);
}

// dWx of both cells = x^T · dZ^T's two column ranges
static int packed_dWx(const Call &c, const PackedBwd &k) {
  const Layout &L = c.L;
  const int P = k.P, G = k.G, D = c.D;
  // x^T: the producer layer's forward kernel wrote it (x_pk_cols; its row maxima were set by this layer's forward
  // call) — or, since the forward call packs x anyway, from that call (res_xT_off) — or one transposing pass over x here
  const void *xTop = L.x_pk ? c.d->x_pk_cols : L.res_xT_off ? c.reserve + L.res_xT_off : k.pk + L.pk_xT;
  if (!L.x_pk && !L.res_xT_off)
    NABU_TRY(pk_pack_any(P, 1, c.x, D, k.M, D, k.pk + L.pk_xT, k.rpD, 0, 0, k.rpD, k.nkbT, 0, 0, k.axT, c.stream));
  nabu_pk_gemm_desc g = pk_desc(P, D, 2 * G, k.nkbT, xTop, k.rpD, k.dzTp, k.rpG, c.dkern[0], G);
  g.C2[0] = c.dkern[1]; g.n_split = G;
  // direct = 2: the three plane products chained directly into the accumulators wherever that rounds less often
  // than the exact-fp32 kernel would (gemm_pk.hip; 0.6-0.8 x its error at these shapes, tests/test_hip_gemm_pk.py)
  if (P == 2) { g.a_amax[0] = k.axT; g.b_amax[0] = k.adzT; g.direct = 2; }
  return nabu_gemm_pk(&g, c.w + L.gemm_off, L.gemm_bytes, c.stream);
}

// dWh = h_{t-1}^T · dZ: the forward cell pairs dz[b,t] with out[b,t-1,:H], the backward cell with out[b,t+1,H:].
// Narrow input (the first layer, D = 40; pk_whole): x^T sits in front of h^T in the same operand and the whole kernel
// gradient [(D+H), 4H] of a cell is ONE product (its dWx alone cost more on the in-kernel-split kernel)
static int packed_dWh(const Call &c, const PackedBwd &k) {
  const Layout &L = c.L;
  const int P = k.P, G = k.G, M = k.M, D = c.D, H = c.H, T = c.T;
  const float *x = c.x, *out = c.h;
  const int r0 = L.pk_whole ? D : 0, Mw = r0 + H, rpW = nabu_pk_rows_pad(Mw);
  // h^T: in the caller's hT_pk, written by the forward call (ABI version 3) — or packed here from `out`
  char *hTb[2] = {k.pk + L.pk_hT[0], k.pk + L.pk_hT[1]};
  if (L.hT_ext) { hTb[0] = static_cast<char *>(c.d->hT_pk); hTb[1] = hTb[0] + L.cmp_bytes[2] / 2; }
  uint32_t *ahT[2] = {k.ahT[0], k.ahT[1]};
  if (P == 2 && L.res_ahT_off) {   // |h| <= 1: the bound sits in the reserve since the forward call (both cells share it)
    ahT[0] = ahT[1] = c.in_reserve<uint32_t>(L.res_ahT_off);
  } else if (P == 2) {   // |h| <= 1 by construction (o · tanh c): one fill for both cells; the input features' maxima
    // are the ones every forward call keeps (x_colmax_kept: copied into place by the same fill) or are measured here
    const unsigned hb = L.hT_ext ? CMP_AMAX_BITS : bound_bits(1.0f);
    const uint32_t *kept = L.x_colmax_kept ? c.in_reserve<uint32_t>(L.res_axT_off) : nullptr;
    const FillSeg fill[4] = {{ahT[0], (size_t)r0, 0u, kept}, {ahT[0] + r0, (size_t)(rpW - r0), hb},
                             {ahT[1], (size_t)r0, 0u, kept}, {ahT[1] + r0, (size_t)(rpW - r0), hb}};
    // (r0 = D is a multiple of 4: every region starts 16-byte aligned)
    NABU_TRY(multi_fill(fill, 4, c.s));
    if (L.pk_whole && !kept) NABU_TRY(pk_amax_pair(x, nullptr, D, M, D, nullptr, ahT[0], nullptr, ahT[1], c.s));
  }
  {   // [x^T ;] h^T of both cells: one launch
    PkPackReq rq[4];
    int n = 0;
    for (int dir = 0; dir < 2; ++dir) {
      const uint32_t *am = P == 2 ? ahT[dir] : nullptr;
      if (L.pk_whole) rq[n++] = PkPackReq{x, D, M, D, hTb[dir], rpW, 0, 0, D, k.nkbT, 0, 0, am};
      if (!L.hT_ext)
        rq[n++] = PkPackReq{out + (size_t)dir * H, 2 * H, M, H, hTb[dir], rpW, r0, 0, rpW - r0, k.nkbT, T, dir ? 1 : -1, am};
    }
    if (n) NABU_TRY(pk_pack_multi(P, 1, rq, n, c.s));
  }
  nabu_pk_gemm_desc g = pk_desc(P, Mw, G, k.nkbT, hTb[0], rpW, k.dzTp, k.rpG, c.dkern[0] + (size_t)(D - r0) * G, G);
  g.nbatch = 2; g.A[1] = hTb[1]; g.B[1] = k.dzTp + (size_t)G * 32; g.C[1] = c.dkern[1] + (size_t)(D - r0) * G;
  if (P == 2) { g.a_amax[0] = ahT[0]; g.a_amax[1] = ahT[1]; g.b_amax[0] = k.adzT; g.b_amax[1] = k.adzT + G; g.direct = 2; }
  return nabu_gemm_pk(&g, c.w + L.gemm_off, L.gemm_bytes, c.stream);
}

static int packed_products(int parts, const Call &c, PersistOut *po) {
  const Layout &L = c.L;
  const PackedBwd k(c);
  if (parts & 1) {
    NABU_TRY(pack_dz(c, k, po));
    if (c.d_x && L.pk_in) NABU_TRY(packed_dx(c, k));
  }
  if ((parts & 2) && L.pk_in) NABU_TRY(packed_dWx(c, k));
  if ((parts & 2) && L.pk_rec) NABU_TRY(packed_dWh(c, k));
  return 0;
}

// ---------------------------------------------------------------------------
// stages: one direction's products on row-major operands — whatever of them the packed path did not take — and the
// plain cell's bias gradient
static int plain_weight_products(const Call &c, int dir) {
  const Layout &L = c.L;
  const int B = c.B, T = c.T, D = c.D, H = c.H, M = B * T;
  // dWx = x^T · dz
  if (!L.pk_in && !L.pk_whole)
    NABU_TRY(nabu_gemm_ex(c.d->gemm_precision, 1, 0, D, 4 * H, M, 1.f, c.x, D, c.gates[dir], 4 * H, 0.f, c.dkern[dir], 4 * H,
                          nullptr, 0, 0, 0, c.gemm_ws(), L.gemm_bytes, c.stream));
  // dWh = h_{prev}^T · dz : fw pairs (out[b,t-1,:H], dz[b,t]); bw pairs (out[b,t+1,H:], dz[b,t]); no pair at T = 1
  if (L.pk_rec) return 0;
  float *dWh = c.dkern[dir] + (size_t)D * 4 * H;
  if (T == 1) {
    NABU_HIP(hipMemsetAsync(dWh, 0, (size_t)H * 4 * H * sizeof(float), c.s));
    return 0;
  }
  const float *A = dir == 0 ? c.h : c.h + H + (size_t)2 * H;
  const float *Bm = dir == 0 ? c.gates[0] + (size_t)4 * H : c.gates[1];
  return nabu_gemm_f32(1, 0, H, 4 * H, B * (T - 1), 1.f, A, 2 * H, Bm, 4 * H, 0.f, dWh, 4 * H, nullptr, T - 1,
                       (long long)T * 2 * H, (long long)T * 4 * H, c.gemm_ws(), L.gemm_bytes, c.stream);
}
static int plain_data_products(const Call &c, int dir, const PersistOut &po) {
  const Layout &L = c.L;
  const int D = c.D, H = c.H, M = c.B * c.T;
  if (!c.L.ln) {
    // db = column sums of dz: the persistent kernel already summed them per unit (one launch adds the few partial
    // rows of both cells)
    if (po.db_part) {
      if (!dir && !po.db_done) NABU_TRY(colsum_pair(po.db_rows, 4 * H, po.db_part, 2 * 4 * H, c.cell.dbias[0], c.cell.dbias[1], c.s));
    } else {
      NABU_TRY(nabu_colsum_f32(M, 4 * H, c.gates[dir], 4 * H, 0.f, c.cell.dbias[dir], c.gemm_ws(), L.gemm_bytes, c.stream));
    }
  }
  // dx (+)= dz · Wx^T
  if (c.d_x && !L.pk_in)
    NABU_TRY(nabu_gemm_ex(c.d->gemm_precision, 0, 1, M, D, 4 * H, 1.f, c.gates[dir], 4 * H, c.kern[dir], 4 * H,
                          dir == 0 ? 0.f : 1.f, c.d_x, D, nullptr, 0, 0, 0, c.gemm_ws(), L.gemm_bytes, c.stream));
  return 0;
}

// THE BACKWARD PASS of a layer, either cell.  parts: 1 = data (recurrence backward, bias resp. norm-parameter
// gradients, input gradient, the packs of dz), 2 = weights (dWx, dWh from the dz the data part left in the reserve),
// 3 = both
static int blstm_backward(int parts, const DescScope &scope, const Cell &cell, const float *x, const int32_t *len,
                          const float *kernel_fw, const float *kernel_bw, const float *out, const float *d_out, void *reserve,
                          float *d_x, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  if (scope.err) return scope.err;
  const nabu_blstm_desc *d = &scope.d;
  const char *who = ENTRY[scope.ln][parts];
  const Layout L = make_layout(d, scope.ln);
  NABU_CHECK_ARG(x && len && out && reserve && ws, "%s: null pointer", who);
  if (parts & 1) {
    NABU_CHECK_ARG(kernel_fw && kernel_bw && d_out, "%s: null pointer", who);
    NABU_TRY(check_cell(L, cell, true, who));
  }
  if (parts & 2) NABU_CHECK_ARG(dkernel_fw && dkernel_bw, "%s: null pointer", who);
  NABU_TRY(tag_check(d, L, reserve, who));
  if (ws_bytes < L.total) return fail(NABU_EWS, "%s: workspace %zu < %zu", who, ws_bytes, L.total);
  if (d->mode == NABU_LSTM_PERSISTENT && !L.plan.supported)
    return fail(NABU_EUNSUP, "%s: persistent kernel does not support B=%d H=%d", who, d->B, d->H);
  Call c(d, L, cell, x, len, kernel_fw, kernel_bw, reserve, ws, stream);
  c.h = out; c.d_out = d_out; c.d_x = d_x; c.dkern[0] = dkernel_fw; c.dkern[1] = dkernel_bw;

  PersistOut po = {};
  if (L.pk_planes == 2 && L.pk_in && d_x && L.pk_rowmax_bytes) po.rowmax = reinterpret_cast<uint32_t *>(c.w + L.pk_off + L.pk_rowmax);
  if (parts & 1) {
    // dz rows of frames never visited by the recurrence must be zero
    for (int dir = 0; dir < 2; ++dir) NABU_TRY(zero_unvisited_frames(c, c.gates[dir], 4 * (size_t)c.H));
    NABU_TRY(recurrence_bwd(c, &po));
    if (L.ln) NABU_TRY(ln_param_grads(ln_args(c), cell.ln, c.s));
  }
  // weight / input gradients from dz (now stored in gates[])
  if (L.pk_planes) NABU_TRY(packed_products(parts, c, &po));
  // The same two per-direction functions in two orders, ONLY so that every launch stays where the two former drivers
  // had it (LABNOTES.md, section 15): the layer-norm driver finished the data part before the weight part, the plain
  // one walked the directions once.  All of these products are independent but for dx of the second direction, which
  // accumulates onto the first's in either order.
  if (L.ln) {
    for (int dir = 0; dir < 2 && (parts & 1); ++dir) NABU_TRY(plain_data_products(c, dir, po));
    for (int dir = 0; dir < 2 && (parts & 2); ++dir) NABU_TRY(plain_weight_products(c, dir));
  } else {                  // one walk over the directions
    for (int dir = 0; dir < 2; ++dir) {
      if (parts & 2) NABU_TRY(plain_weight_products(c, dir));
      if (parts & 1) NABU_TRY(plain_data_products(c, dir, po));
    }
  }
  return 0;
}

}  // namespace nabu

using namespace nabu;

extern "C" int nabu_blstm_set_profile_events(void *ev_begin, void *ev_end) {
  g_ev_begin = static_cast<hipEvent_t>(ev_begin);
  g_ev_end = static_cast<hipEvent_t>(ev_end);
  return 0;
}
extern "C" int nabu_blstm_set_phase_hook(nabu_phase_hook_t fn, void *user) {
  g_phase_hook = fn;
  g_phase_user = user;
  return 0;
}
extern "C" int nabu_persist_set_timeout_us(long long us) {
  nabu::lstm_persist_set_timeout_us(us);
  return 0;
}

// ---- the queries: 0 for a descriptor the family refuses
extern "C" int nabu_blstm_uses_persistent(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, false);
  return !scope.err && use_persistent(&scope.d, plan_of(&scope.d)) ? 1 : 0;
}
extern "C" int nabu_blstm_pk_bytes(const nabu_blstm_desc *d_in, size_t bytes[5]) {
  const DescScope scope(d_in, false);
  if (scope.err) return scope.err;
  NABU_CHECK_ARG(bytes, "blstm_pk_bytes: null pointer");
  const Layout L = make_layout(&scope.d, false);
  for (int i = 0; i < 5; ++i) bytes[i] = L.cmp_bytes[i];
  return 0;
}
extern "C" int nabu_blstm_emits_packed(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, false);
  return scope.err ? 0 : emitted_by_kernel(&scope.d, make_layout(&scope.d, false));
}
extern "C" size_t nabu_blstm_reserve_bytes(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, false);
  return scope.err ? 0 : make_layout(&scope.d, false).reserve_bytes;
}
extern "C" size_t nabu_blstm_ws_bytes(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, false);
  return scope.err ? 0 : make_layout(&scope.d, false).total;
}
extern "C" size_t nabu_blstm_ln_reserve_bytes(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, true);
  return scope.err ? 0 : make_layout(&scope.d, true).reserve_bytes;
}
extern "C" size_t nabu_blstm_ln_ws_bytes(const nabu_blstm_desc *d_in) {
  const DescScope scope(d_in, true);
  return scope.err ? 0 : make_layout(&scope.d, true).total;
}

// ---- the plain cell
extern "C" int nabu_blstm_fwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len,
                              const float *kernel_fw, const float *bias_fw,
                              const float *kernel_bw, const float *bias_bw, float *out,
                              void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return blstm_forward(DescScope(d_in, false), plain_cell(bias_fw, bias_bw, nullptr, nullptr), x, len, kernel_fw, kernel_bw, out,
                       reserve, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_bwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len,
                              const float *kernel_fw, const float *kernel_bw, const float *out,
                              const float *d_out, void *reserve, float *d_x, float *dkernel_fw,
                              float *dbias_fw, float *dkernel_bw, float *dbias_bw, void *ws,
                              size_t ws_bytes, nabu_stream_t stream) {
  return blstm_backward(3, DescScope(d_in, false), plain_cell(nullptr, nullptr, dbias_fw, dbias_bw), x, len, kernel_fw, kernel_bw,
                        out, d_out, reserve, d_x, dkernel_fw, dkernel_bw, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_bwd_data(const nabu_blstm_desc *d_in, const float *x, const int32_t *len,
                                   const float *kernel_fw, const float *kernel_bw, const float *out,
                                   const float *d_out, void *reserve, float *d_x, float *dbias_fw, float *dbias_bw,
                                   void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return blstm_backward(1, DescScope(d_in, false), plain_cell(nullptr, nullptr, dbias_fw, dbias_bw), x, len, kernel_fw, kernel_bw,
                        out, d_out, reserve, d_x, nullptr, nullptr, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_bwd_weights(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *out,
                                      void *reserve, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                                      nabu_stream_t stream) {
  return blstm_backward(2, DescScope(d_in, false), plain_cell(nullptr, nullptr, nullptr, nullptr), x, len, nullptr, nullptr, out,
                        nullptr, reserve, nullptr, dkernel_fw, dkernel_bw, ws, ws_bytes, stream);
}

// ---- the layer-normalised cell
extern "C" int nabu_blstm_ln_fwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *kernel_fw,
                                 const float *kernel_bw, const nabu_blstm_ln_params *ln, float *out, void *reserve,
                                 void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return blstm_forward(DescScope(d_in, true), ln_cell(ln), x, len, kernel_fw, kernel_bw, out, reserve, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_ln_bwd(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *kernel_fw,
                                 const float *kernel_bw, const nabu_blstm_ln_params *ln, const float *out,
                                 const float *d_out, void *reserve, float *d_x, float *dkernel_fw, float *dkernel_bw,
                                 void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return blstm_backward(3, DescScope(d_in, true), ln_cell(ln), x, len, kernel_fw, kernel_bw, out, d_out, reserve, d_x, dkernel_fw,
                        dkernel_bw, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_ln_bwd_data(const nabu_blstm_desc *d_in, const float *x, const int32_t *len,
                                      const float *kernel_fw, const float *kernel_bw, const nabu_blstm_ln_params *ln,
                                      const float *out, const float *d_out, void *reserve, float *d_x, void *ws,
                                      size_t ws_bytes, nabu_stream_t stream) {
  return blstm_backward(1, DescScope(d_in, true), ln_cell(ln), x, len, kernel_fw, kernel_bw, out, d_out, reserve, d_x, nullptr,
                        nullptr, ws, ws_bytes, stream);
}
extern "C" int nabu_blstm_ln_bwd_weights(const nabu_blstm_desc *d_in, const float *x, const int32_t *len, const float *out,
                                         void *reserve, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                                         nabu_stream_t stream) {
  return blstm_backward(2, DescScope(d_in, true), ln_cell(nullptr), x, len, nullptr, nullptr, out, nullptr, reserve, nullptr,
                        dkernel_fw, dkernel_bw, ws, ws_bytes, stream);
}
