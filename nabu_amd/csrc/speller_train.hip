// speller_train.hip — whole-sequence training driver of the Speller decoder, for 1..M memories.
//
// The per-step launch sequence of RNNDecoder._decode runs here, in C++, so that a decoder step costs its kernel
// launches only (a Python/ctypes loop spent ~15 us of host time per launch).  The kernels live elsewhere: cell and
// one-memory attention in speller.hip, the M-mechanism attention launch in speller_multi.hip, the persistent decoder
// in speller_persist.hip, the skinny products in gemm_skinny.hip.
//
// One driver serves nabu_speller_* and nabu_speller_multi_*: the two descriptors become one geometry (SpGeo), ONE
// function decides the path of the call (speller_plan, speller_plan.h) and the passes are made of named stages that
// read the plan's fields.  The families differ in the attention step — attn_fwd_impl / attn_bwd_impl for
// nabu_speller_*, ONE multi launch per step and pass for nabu_speller_multi_* (also with M = 1) — and in plan fields:
// the persistent decoder, rows16 products, cell epilogues, deferred attention gradients and sub-batch streams are
// off for the multi family, and its generic backward chain multiplies against the parameters themselves.
#include "common.h"
#include "gemm_args.h"
#include "speller_attn.h"
#include "speller_plan.h"

#include <stdlib.h>

#include <string>
#include <thread>

namespace nabu {

namespace {

constexpr int MM = NABU_SPELLER_MAX_MEMORIES, ML = NABU_SPELLER_MAX_LAYERS;

// ---------------------------------------------------------------------------
// check + normalise: the two descriptor families as one SpGeo

int check_sp(const nabu_speller_desc *d) {
  if (!d || d->size != sizeof(nabu_speller_desc)) return fail(NABU_EINVAL, "speller: bad descriptor size");
  if (d->B <= 0 || d->Te <= 0 || d->E <= 0 || d->U <= 0 || d->C <= 1 || d->L <= 0)
    return fail(NABU_EINVAL, "speller: bad dimensions");
  if (d->num_layers < 1 || d->num_layers > ML) return fail(NABU_EUNSUP, "speller: 1..%d layers", ML);
  if (d->U % 4 || d->E % 4) return fail(NABU_EUNSUP, "speller: num_units and encoder dim must be multiples of 4");
  if (!(d->keep_prob > 0.f && d->keep_prob <= 1.f)) return fail(NABU_EINVAL, "speller: keep_prob out of (0,1]");
  if (!(d->sample_prob >= 0.f && d->sample_prob <= 1.f)) return fail(NABU_EINVAL, "speller: sample_prob out of [0,1]");
  nabu_attn_desc a = {sizeof(nabu_attn_desc), d->B, d->Te, d->E, d->U, d->kind, d->K, d->F, d->prob_fn};
  return check_attn(&a);
}

int geo_of(const nabu_speller_desc *d, SpGeo *g) {
  if (int e = check_sp(d)) return e;
  *g = SpGeo{};
  g->d = nabu_speller_multi_desc{sizeof(nabu_speller_multi_desc), 1, d->B, d->U, d->C, d->L, d->num_layers, {d->Te}, {d->E},
                                 d->kind, d->K, d->F, d->prob_fn, d->keep_prob, d->seed, d->seed_offset, d->sample_prob,
                                 d->sample_seed, d->sample_offset};
  g->a.M = 1; g->a.SE = d->E; g->a.MU = d->U;
  return 0;
}
int geo_of(const nabu_speller_multi_desc *d, SpGeo *g) {
  *g = SpGeo{};
  g->multi = true;
  if (int e = multi_attn_geo(d, &g->a)) return e;
  g->d = *d;
  return 0;
}

void operands(SpGeo *g, const float *values, const int32_t *enc_len, const int32_t *ids, const int32_t *dec_len,
              const nabu_speller_params *p, const nabu_speller_grads *gr, float *dvalues) {
  g->values[0] = values; g->enc_len[0] = enc_len; g->ids = ids; g->dec_len = dec_len; g->dvalues[0] = dvalues;
  g->p.memory_kernel[0] = p->memory_kernel; g->p.query_kernel[0] = p->query_kernel; g->p.attention_v[0] = p->attention_v;
  g->p.conv_kernel[0] = p->conv_kernel; g->p.conv_proj[0] = p->conv_proj;
  g->p.out_kernel = p->out_kernel; g->p.out_bias = p->out_bias;
  for (int n = 0; n < ML; ++n) { g->p.lstm_kernel[n] = p->lstm_kernel[n]; g->p.lstm_bias[n] = p->lstm_bias[n]; }
  if (!gr) return;
  g->gr.memory_kernel[0] = gr->memory_kernel; g->gr.query_kernel[0] = gr->query_kernel; g->gr.attention_v[0] = gr->attention_v;
  g->gr.conv_kernel[0] = gr->conv_kernel; g->gr.conv_proj[0] = gr->conv_proj;
  g->gr.out_kernel = gr->out_kernel; g->gr.out_bias = gr->out_bias;
  for (int n = 0; n < ML; ++n) { g->gr.lstm_kernel[n] = gr->lstm_kernel[n]; g->gr.lstm_bias[n] = gr->lstm_bias[n]; }
}
// nabu_speller_multi_params | nabu_speller_multi_grads (the same fields), with the memories or their gradients
template <typename P>
int check_ptrs(const nabu_speller_multi_desc &d, const float *const *values, const int32_t *const *enc_len, const P &p) {
  for (int m = 0; m < d.M; ++m) {
    NABU_CHECK_ARG(values[m] && enc_len[m] && p.memory_kernel[m] && p.query_kernel[m] && p.attention_v[m],
                   "speller_multi: null pointer for an encoded input");
    NABU_CHECK_ARG(d.kind != 1 || (p.conv_kernel[m] && p.conv_proj[m]),
                   "speller_multi: location-aware attention needs its kernels");
  }
  NABU_CHECK_ARG(p.out_kernel && p.out_bias, "speller_multi: null pointer");
  for (int n = 0; n < d.num_layers; ++n) NABU_CHECK_ARG(p.lstm_kernel[n] && p.lstm_bias[n], "speller_multi: null pointer");
  return 0;
}
int operands(SpGeo *g, const float *const *values, const int32_t *const *enc_len, const int32_t *ids, const int32_t *dec_len,
             const nabu_speller_multi_params *p, const nabu_speller_multi_grads *gr, float *const *dvalues) {
  NABU_TRY(check_ptrs(g->d, values, enc_len, *p));
  if (gr) NABU_TRY(check_ptrs(g->d, dvalues, enc_len, *gr));
  for (int m = 0; m < g->d.M; ++m) {
    g->values[m] = values[m]; g->enc_len[m] = enc_len[m];
    if (gr) g->dvalues[m] = dvalues[m];
  }
  g->ids = ids; g->dec_len = dec_len; g->p = *p;
  if (gr) g->gr = *gr;
  return 0;
}

nabu_attn_desc attn_desc(const SpGeo &g, int m, int rows) {
  nabu_attn_desc a = {sizeof(nabu_attn_desc), rows, g.d.Te[m], g.d.E[m], g.d.U, g.d.kind, g.d.K, g.d.F, g.d.prob_fn};
  return a;
}

// ---------------------------------------------------------------------------
// the reserve (what the forward pass keeps for the backward pass): offsets in floats.  Every item is rounded to 4
// floats by itself, so the total does not depend on the order.
struct SpReserve {
  size_t H[ML], Cs[ML], Ho[ML], acts[ML];
  size_t ctx, q, logits_tm, ids, align[MM], keys[MM], znorm[MM], total;   // (ids: [L,B] int32)
  size_t dscale, sdraw;    // persistent decoder (speller_persist.h): dropout scale factors [L,B,U], sampling draws [L,B,2]
};
SpReserve sp_reserve(const SpGeo &g) {
  SpReserve s = {};
  const size_t B = g.d.B, L = g.d.L, U = g.d.U, C = g.d.C;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += (n + 3) / 4 * 4; return r; };
  for (int n = 0; n < g.d.num_layers; ++n) {
    s.H[n] = take((L + 1) * B * U);
    s.Cs[n] = take((L + 1) * B * U);
    s.Ho[n] = g.d.keep_prob < 1.f ? take((L + 1) * B * U) : s.H[n];
    s.acts[n] = take(L * B * 4 * U);
  }
  s.ctx = take((L + 1) * B * g.a.SE);
  s.q = take(L * B * g.a.MU);
  s.logits_tm = take(L * B * C);
  s.ids = take(L * B);
  for (int m = 0; m < g.d.M; ++m) {
    s.align[m] = take((L + 1) * B * g.d.Te[m]);
    s.keys[m] = take(B * g.d.Te[m] * U);
    s.znorm[m] = take(L * B);
  }
  if (!g.multi) {
    s.dscale = g.d.keep_prob < 1.f ? take(L * B * U) : 0;
    s.sdraw = g.d.sample_prob > 0.f ? take(2 * L * B) : 0;
  }
  s.total = o;
  return s;
}

// ---------------------------------------------------------------------------
// THE PLAN (speller_plan.h)
// shapes gemm_skinny_fused takes: C[M,N] = A·B + A2·B2 in ONE launch with the split-K reduction inside it
bool fused_shape(int M, int N, int K1, int lda, int K2, int lda2) {
  return M <= 64 && N % 32 == 0 && K1 > 0 && K1 % 64 == 0 && K2 % 64 == 0 && lda % 4 == 0 && (K2 == 0 || lda2 % 4 == 0);
}
// The L decoder steps are a chain of small dependent kernels (each ~5 us of launch + memory latency,
// whatever its size).  Utterances are independent of each other until the weight gradients are summed, so
// the batch is cut into NS sub-batches whose chains run concurrently on NS streams (forked from / joined
// to the caller's stream by events); what one chain leaves idle the others use.  NABU_SPELLER_STREAMS=n
// overrides (1 = off).
int sub_batches(int B, int env) {
  int want = env > 0 ? env : 4;
  while (want > 1 && (B % want != 0 || B / want < (env > 0 ? 1 : 16))) want /= 2;
  return want < 1 ? 1 : want;
}

// (reserve: null in the size queries; the persistent launches find their random-number arrays in it)
SpellerPlan speller_plan(const SpGeo &g, float *reserve) {
  SpellerPlan P = {};
  const auto &d = g.d;
  const int B = d.B, U = d.U, E = d.E[0], C = d.C, nl = d.num_layers;
  P.NS = 1; P.Bn = B;
  if (g.multi) return P;          // one chain of generic products on the caller's stream
  P.NS = sub_batches(B, env_int("NABU_SPELLER_STREAMS", 0));
  const int Bn = P.Bn = B / P.NS;
  P.threads = env_int("NABU_SPELLER_THREADS", 0) != 0;
  P.fused = env_int("NABU_SPELLER_FUSED", 1) != 0;
  P.tickets = env_int("NABU_SPELLER_ATTN_FUSED", 1) != 0;
  P.weights_T = true;
  const bool epi = env_int("NABU_SPELLER_EPILOGUE", 1) && P.fused, rows16_on = env_int("NABU_SPELLER_ROWS16", 1),
             split_on = env_int("NABU_SPELLER_SPLIT", 1), defer_on = env_int("NABU_SPELLER_DEFER", 1);
  const nabu_attn_desc adn = attn_desc(g, 0, Bn), adb = attn_desc(g, 0, B);
  P.S = attn_bwd_nslices(&adn);
  const bool drop = d.keep_prob < 1.f;

  const SpReserve R = sp_reserve(g);
  SpPersistDesc &pd = P.pd;
  pd = SpPersistDesc{B, d.L, U, E, d.Te[0], C};
  pd.kind = d.kind; pd.K = d.K; pd.F = d.F;
  pd.keep_prob = d.keep_prob; pd.seed = d.seed; pd.seed_offset = d.seed_offset;     // nl == 1: offset + t*nl + n = offset + t
  pd.sample_prob = d.sample_prob; pd.sample_seed = d.sample_seed; pd.sample_offset = d.sample_offset;
  pd.drop_scale = (drop && reserve) ? reserve + R.dscale : nullptr;
  pd.sample_draws = (d.sample_prob > 0.f && reserve) ? reinterpret_cast<unsigned *>(reserve + R.sdraw) : nullptr;
  P.pd_bwd = pd;
  P.pd_bwd.sample_prob = 0.f; P.pd_bwd.sample_seed = P.pd_bwd.sample_offset = 0; P.pd_bwd.sample_draws = nullptr;
  P.persist_bytes = speller_persist_ws_bytes(P.pd_bwd);
  const size_t bwd_bytes = speller_persist_bwd_ws_bytes(P.pd_bwd);
  if (bwd_bytes > P.persist_bytes) P.persist_bytes = bwd_bytes;
  P.persist_bwd_shape = bwd_bytes > 0;
  const bool persist_kind = (d.kind == 0 || d.kind == 1) && d.prob_fn == 0 && P.persist_bytes > 0;

  // forward.  LSTM cell folded into the step product's last workgroup (gemm_skinny.hip) when the shapes allow: the
  // product then runs against gate-interleaved copies of the kernels' dense rows
  for (int n = 0; n < nl; ++n) {
    const int K1 = n == 0 ? E : U;
    P.cell_epi[n] = epi && fused_shape(Bn, 4 * U, K1, K1, U, U);
  }
  const bool rows16_f = rows16_on && E % 16 == 0 && rows16_ok(Bn, 4 * U, E + U, E) && rows16_ok(Bn, U, U, U);
  // the whole step loop as ONE persistent launch where the geometry allows: one LSTM layer, vanilla or location-aware
  // softmax attention, B = 32 or 64
  P.fwd.persist = nl == 1 && persist_kind && P.cell_epi[0] && speller_persist_ok(pd);
  if (P.fwd.persist) {
    // Location-aware attention, more than one launch of 32 utterances, values streamed from L2 (cfg5's geometry): the step
    // chain on sub-batches of 16 with its round-5 kernels (rows16_kernel, attn_fwd_loc_mfma_kernel) is faster than two
    // persistent launches (cfg5: 41.0 against 42.7 ms per training step).  NABU_SPELLER_PERSIST=2: the persistent kernel anyway.
    const bool chain_fast = d.kind == 1 && B > 32 && Bn <= 64 && (d.sample_prob == 0.f || sample_step_ok(C)) && rows16_f &&
                            speller_persist_streams_values(pd);
    if (chain_fast && env_int("NABU_SPELLER_PERSIST", 1) != 2) P.fwd.persist = false;
  }
  // sub-batches of <= 16 utterances: the cell's product ([context | h] . kernel with the cell as epilogue) and the query
  // by rows16_kernel over weights re-blocked once per pass; NABU_SPELLER_ROWS16=0: gemm_skinny_fused
  P.fwd.r16 = !P.fwd.persist && nl == 1 && P.cell_epi[0] && rows16_f;

  // backward.  Single-layer decoder: the cell's backward pass is folded into the last workgroup of dq·Wq^T, and
  // dz·[Kx^T | Kh^T] is ONE product whose [B, E+U] result carries d context and d h to the next step — 4 dependent
  // launches per step instead of 7
  const bool fuse_shapes = epi && nl == 1 && fused_shape(Bn, U, U, U, 0, 0) && fused_shape(Bn, E + U, 4 * U, 4 * U, 0, 0) &&
                           (E + U) / 32 <= 1024;
  const int Sp = defer_on ? attn_defer_slices(&adb) : 0;
  // (location-aware attention: the persistent kernel leaves d keys / d attention_v / d conv_proj to attn_param_grads_kernel)
  P.bwd.persist = (d.kind != 1 || Sp > 0) && fuse_shapes && persist_kind && speller_persist_bwd_ok(P.pd_bwd);
  // both products of a step by rows16_kernel (no split-K hand-off between workgroups: 13 -> 7 us per launch; its cell
  // epilogue applies the output dropout's mask)
  P.bwd.r16 = fuse_shapes && !P.bwd.persist && E % 32 == 0 && split_on && rows16_on && rows16_ok(Bn, U, U, U) &&
              rows16_ok(Bn, E + U, 4 * U, 4 * U);
  P.fuse_b = fuse_shapes && (!drop || P.bwd.persist || P.bwd.r16);      // (gemm_skinny_fused's cell epilogue has no dropout)
  P.split_b = P.fuse_b && E % 32 == 0 && split_on;
  // d keys / d attention_v / d conv_proj of all steps in ONE launch after the chain (the persistent kernel accumulates
  // them itself for vanilla attention)
  P.Sp = (!P.bwd.persist || d.kind == 1) ? Sp : 0;
  return P;
}

// ---------------------------------------------------------------------------
// the workspace: offsets in floats, every item rounded to 4 floats by itself
struct SpWs {
  size_t z, dl, dH, dCtx, dq, dz[ML], dh[2][ML], dc[2][ML], dctx[2], dx, tmp, gemm, gemm_bytes, gemm_each, total;
  size_t dkeys[MM], dv[MM], dwf[MM], dck[MM], dal[2][MM];   // per memory
  size_t tickets, tickets_n;   // zeroed per call
  // ---- nabu_speller_* only
  size_t attn, attn_each;  // the attention calls' scratch, per chain
  size_t wqT, kxT[ML], khT[ML];   // transposed weights (generic backward chain)
  size_t kperm[ML];        // gate-interleaved copies of the cell kernels' dense rows (forward)
  size_t kxhT, dxh[2];     // [4U, E+U] transposed rows of layer 0's kernel; [B, E+U] carries d(context | h) of a step
  size_t wq_sw, kxh_sw;    // the same two weights re-blocked for rows16_kernel: [U, U], [E+U, 4U]
  size_t fpart, fpart_each;   // fused skinny products: partial tiles per chain (their tickets: 1024 per chain, then one per utterance)
  size_t status, persist;  // persistent decoder kernel: status word (ws[0]), XCC table + exchange rings
  size_t dv8, dck8;        // its d attention_v / d conv kernel partial rows [B*8, U], [B*8, K*F]
  size_t ds_all, cf_all;   // deferred attention gradients: d scores [L,B,Te], location features [L,B,Te,F]
  size_t dv16, dwf16;      // ... and the partial rows of attn_param_grads_kernel [B*Sp, U], [B*Sp, F*U]
  // ---- nabu_speller_multi_* only
  size_t wqcat, part[MM], dcf[MM];   // [U, M U] query kernels side by side; the launch's partials and d location features
};
SpWs sp_ws(const SpGeo &g, const SpellerPlan &P) {
  SpWs s = {};
  const auto &d = g.d;
  const size_t B = d.B, L = d.L, U = d.U, C = d.C, SE = g.a.SE, MU = g.a.MU, NS = P.NS, Bn = P.Bn;
  const bool loc = d.kind == 1;
  // (the one-memory sizes count the descriptor's K and F whatever the attention kind)
  const size_t F = g.multi && !loc ? 0 : d.F, K = g.multi && !loc ? 0 : d.K;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += (n + 3) / 4 * 4; return r; };
  if (!g.multi) {
    // ws[0]: status word of the persistent decoder kernel (0 = ok; sticky, the caller provides the workspace
    // zero-initialised once, like the recurrent layers' workspace), then its XCC table and exchange rings
    const size_t Te = d.Te[0];
    s.status = take(64);
    s.persist = take(P.persist_bytes / 4 + 4);
    s.dv8 = take(P.persist_bwd_shape ? B * 8 * U : 0);
    s.dck8 = take((P.persist_bwd_shape && loc) ? B * 8 * K * F : 0);
    s.ds_all = take(L * B * Te);
    s.cf_all = take(loc ? L * B * Te * F : 0);
    s.dv16 = take(B * 16 * U);
    s.dwf16 = take(loc ? B * 16 * F * U : 0);
  }
  s.z = take(B * 4 * U);
  s.dl = take(L * B * C);
  s.dH = take(L * B * U);
  s.dCtx = take(L * B * SE);
  s.dq = take(L * B * MU);
  for (int n = 0; n < d.num_layers; ++n) {
    s.dz[n] = take(L * B * 4 * U);
    for (int i = 0; i < 2; ++i) { s.dh[i][n] = take(B * U); s.dc[i][n] = take(B * U); }
  }
  s.dctx[0] = take(B * SE);                            // d context carried to step t - 1 (generic chain)
  s.dctx[1] = g.multi ? s.dctx[0] : take(B * SE);
  s.dx = take(B * U);
  s.tmp = take(B * U);
  size_t gw = 0;
  auto mx = [&](size_t v) { if (v > gw) gw = v; };
  const int Bi = (int)B, Ui = (int)U, Ci = (int)C, BL = (int)(B * L), SEi = (int)SE, MUi = (int)MU;
  for (int m = 0; m < d.M; ++m) {
    const size_t Te = d.Te[m], E = d.E[m], S = g.multi ? g.a.S[m] : P.S;
    s.dkeys[m] = take(B * Te * U);
    s.dv[m] = take(B * S * U);
    s.dwf[m] = take(B * S * F * U + 4);
    s.dck[m] = take(B * K * F + 4);
    for (int i = 0; i < 2; ++i) s.dal[i][m] = take(B * Te);
    const int BT = (int)(B * Te), Ei = (int)E;
    mx(nabu_gemm_ws_bytes(BT, Ui, Ei)); mx(nabu_gemm_ws_bytes(BT, Ei, Ui)); mx(nabu_gemm_ws_bytes(Ei, Ui, BT));
    if (g.multi) {
      s.part[m] = take(B * S * (E + 4 > U ? E + 4 : U));
      s.dcf[m] = take(B * Te * F + 4);
      mx(nabu_colsum_ws_bytes((int)(B * S), (int)(F * U + U))); mx(nabu_colsum_ws_bytes(Bi, (int)(K * F + 4)));
    }
  }
  if (g.multi) {
    s.wqcat = take(U * MU);
    s.tickets_n = (size_t)MM * B;
    s.tickets = take(s.tickets_n);
    mx(nabu_colsum_ws_bytes(BL, Ci));
  } else {
    const size_t E = SE, Te = d.Te[0];
    const nabu_attn_desc adn = attn_desc(g, 0, (int)Bn);
    const size_t ab = nabu_attn_bwd_ws_bytes(&adn), af = nabu_attn_fwd_ws_bytes(&adn);
    s.attn_each = ((ab > af ? ab : af) / 4 + 4 + 3) / 4 * 4;
    s.attn = take(NS * s.attn_each);
    s.wqT = take(U * U);
    for (int n = 0; n < d.num_layers; ++n) {
      s.kxT[n] = take(4 * U * (n == 0 ? E : U));
      s.khT[n] = take(4 * U * U);
    }
    for (int n = 0; n < d.num_layers; ++n) s.kperm[n] = take((n == 0 ? E + U : 2 * U) * 4 * U);
    s.kxhT = take(4 * U * (E + U));
    s.wq_sw = take(U * U);
    s.kxh_sw = take(4 * U * (E + U));
    for (int i = 0; i < 2; ++i) s.dxh[i] = take(B * (E + U));
    s.tickets_n = NS * 1024 + B + 4;   // + one counter per utterance for the attention launches
    s.tickets = take(s.tickets_n);
    const size_t kmax = E + U > 4 * U ? E + U : 4 * U, nmax = 4 * U > E ? 4 * U : E;
    s.fpart_each = ((kmax / 64 + 1) * Bn * nmax + 3) / 4 * 4;
    s.fpart = take(NS * s.fpart_each);
    mx(nabu_gemm_ws_bytes((int)Te, SEi, (int)L));
    mx(nabu_colsum_ws_bytes((int)(B * 16), (int)(F * U + K * F + U)));
  }
  mx(nabu_gemm_ws_bytes(Bi, 4 * Ui, SEi)); mx(nabu_gemm_ws_bytes(Bi, 4 * Ui, Ui)); mx(nabu_gemm_ws_bytes(Bi, MUi, Ui));
  mx(nabu_gemm_ws_bytes(Bi, Ui, MUi)); mx(nabu_gemm_ws_bytes(Bi, SEi, 4 * Ui)); mx(nabu_gemm_ws_bytes(Bi, Ui, 4 * Ui));
  mx(nabu_gemm_ws_bytes(Bi, Ci, Ui)); mx(nabu_gemm_ws_bytes(Bi, Ci, SEi));
  mx(nabu_gemm_ws_bytes(BL, Ci, Ui)); mx(nabu_gemm_ws_bytes(BL, Ci, SEi));
  mx(nabu_gemm_ws_bytes(Ui, Ci, BL)); mx(nabu_gemm_ws_bytes(SEi, Ci, BL));
  mx(nabu_gemm_ws_bytes(BL, Ui, Ci)); mx(nabu_gemm_ws_bytes(BL, SEi, Ci));
  mx(nabu_gemm_ws_bytes(Ui, Ui, BL)); mx(nabu_gemm_ws_bytes(SEi, 4 * Ui, BL)); mx(nabu_gemm_ws_bytes(Ui, 4 * Ui, BL));
  mx(nabu_colsum_ws_bytes(BL, 4 * Ui));
  s.gemm_bytes = (gw + 255) / 256 * 256;
  s.gemm_each = s.gemm_bytes / 4 + 4;
  s.gemm = take(NS * s.gemm_each);
  s.total = o;
  return s;
}

// ---------------------------------------------------------------------------
// sub-batch streams
struct SubStreams {
  int n;
  hipStream_t st[8];
  hipEvent_t fork, done[8];
};
int sub_streams(int n, hipStream_t main, SubStreams *out) {
  static thread_local hipStream_t side[8] = {nullptr};
  static thread_local hipEvent_t ev[9] = {nullptr};
  out->n = n;
  out->st[0] = main;
  for (int i = 1; i < n; ++i) {
    if (!side[i]) NABU_HIP(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
    out->st[i] = side[i];
  }
  for (int i = 0; i <= n && i < 9; ++i)
    if (!ev[i]) NABU_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  out->fork = ev[0];
  for (int i = 1; i < n; ++i) out->done[i] = ev[i];
  return 0;
}
int sub_fork(const SubStreams &ss) {
  if (ss.n == 1) return 0;
  NABU_HIP(hipEventRecord(ss.fork, ss.st[0]));
  for (int i = 1; i < ss.n; ++i) NABU_HIP(hipStreamWaitEvent(ss.st[i], ss.fork, 0));
  return 0;
}
int sub_join(const SubStreams &ss) {
  for (int i = 1; i < ss.n; ++i) {
    NABU_HIP(hipEventRecord(ss.done[i], ss.st[i]));
    NABU_HIP(hipStreamWaitEvent(ss.st[0], ss.done[i], 0));
  }
  return 0;
}
// Enqueue the sub-batch chains from one host thread each (plan.threads): a chain is thousands of launches, and ONE
// thread feeding four streams is about as fast as the GPU drains them (2.5 us per launch against ~10 us kernels, four
// at a time) — measured: with a single enqueuing thread every queue sat idle ~45% of the time waiting for its next
// step.  body(sub) enqueues ALL steps of one sub-batch on its stream and returns a NABU_E* / hipError_t code.
template <typename F>
int run_subs(int NS, bool threads, F body) {
  if (NS == 1) return body(0);
  int codes[8] = {0};
  std::string texts[8];
  if (!threads) {
    int first = 0;                       // every chain is enqueued even after a failure: the caller joins the streams
    for (int i = 0; i < NS; ++i) {
      const int e = body(i);
      if (e && !first) first = e;
    }
    return first;
  }
  int dev = 0;
  NABU_HIP(hipGetDevice(&dev));
  std::thread th[8];
  for (int i = 1; i < NS; ++i)
    th[i] = std::thread([&, i]() {
      if (hipSetDevice(dev) != hipSuccess) { codes[i] = (int)hipErrorInvalidDevice; texts[i] = "hipSetDevice failed in a decoder enqueue thread"; return; }
      codes[i] = body(i);
      if (codes[i]) texts[i] = err_buf();        // the error text is thread-local: hand it to the caller's thread
    });
  codes[0] = body(0);
  for (int i = 1; i < NS; ++i) th[i].join();
  if (codes[0]) return codes[0];
  for (int i = 1; i < NS; ++i)
    if (codes[i]) return fail(codes[i], "%s", texts[i].c_str());
  return 0;
}

// ---------------------------------------------------------------------------
// one call: geometry, plan, layouts, buffers
struct Run {
  const SpGeo &g;
  SpellerPlan P;
  SpReserve R;
  SpWs W;
  float *r, *w, *gw;
  size_t gwb;
  hipStream_t s;
  SubStreams ss;
  nabu_attn_desc adn;            // one-memory family: the attention calls of a chain, their scratch sizes
  size_t attn_fwd_wsb, attn_bwd_wsb;
  int32_t *ids_used() const { return reinterpret_cast<int32_t *>(r + R.ids); }
  unsigned *attn_tickets() const {      // one counter per utterance behind the chains' product tickets
    return P.tickets ? reinterpret_cast<unsigned *>(w + W.tickets) + (size_t)P.NS * 1024 : nullptr;
  }
};
int make_run(const SpGeo &g, void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream, const char *who, Run *x) {
  x->P = speller_plan(g, static_cast<float *>(reserve));
  x->R = sp_reserve(g);
  x->W = sp_ws(g, x->P);
  if (ws_bytes < x->W.total * sizeof(float)) return fail(NABU_EWS, "%s: workspace too small", who);
  x->r = static_cast<float *>(reserve);
  x->w = static_cast<float *>(ws);
  x->gw = x->w + x->W.gemm;
  x->gwb = x->W.gemm_bytes;
  x->s = static_cast<hipStream_t>(stream);
  if (!g.multi) {
    x->adn = attn_desc(g, 0, x->P.Bn);
    x->attn_fwd_wsb = nabu_attn_fwd_ws_bytes(&x->adn);
    x->attn_bwd_wsb = nabu_attn_bwd_ws_bytes(&x->adn);
  }
  return 0;
}
// one chain of the step loop: sub-batch rows [b0, b0 + Bn) on its stream with its slices of the shared scratch
struct Chain {
  int sub, b0;
  hipStream_t hs;
  float *gws;
  const int32_t *dlen;
};
Chain chain_of(const Run &x, int sub) {
  const int b0 = sub * x.P.Bn;
  return Chain{sub, b0, x.ss.st[sub], x.gw + (size_t)sub * x.W.gemm_each, x.g.dec_len + b0};
}

// C[M,N] = A·B + A2·B2 (+ beta*C): ONE launch with the split-K reduction inside it when the plan and the shape
// allow (gemm_skinny.hip), else two plain products
int mm2(const Run &x, const Chain &c, int M, int N, int K1, const float *A, int lda, const float *Bm, int ldb, int K2,
        const float *A2, int lda2, const float *B2, int ldb2, float beta, float *C, int ldc) {
  if (x.P.fused && fused_shape(M, N, K1, lda, K2, lda2))
    return gemm_skinny_fused(M, N, K1, A, lda, Bm, ldb, K2, A2, lda2, B2, ldb2, beta, C, ldc, nullptr,
                             x.w + x.W.fpart + (size_t)c.sub * x.W.fpart_each,
                             reinterpret_cast<unsigned *>(x.w + x.W.tickets) + (size_t)c.sub * 1024, c.hs);
  if (int e = mm(false, false, M, N, K1, A, lda, Bm, ldb, beta, C, ldc, nullptr, c.gws, x.gwb, c.hs)) return e;
  if (K2 > 0) return mm(false, false, M, N, K2, A2, lda2, B2, ldb2, 1.f, C, ldc, nullptr, c.gws, x.gwb, c.hs);
  return 0;
}
// generic backward chain: C[M,N] = A[M,K] · W^T (+ beta*C), W [N,K] (row stride ldw) a parameter block and WT [K,N]
// its transposed copy of this pass — the plan says which of the two forms is multiplied
int mmT(const Run &x, const Chain &c, int M, int N, int K, const float *A, int lda, const float *WT, const float *Wm, int ldw,
        float beta, float *C, int ldc) {
  if (x.P.weights_T) return mm2(x, c, M, N, K, A, lda, WT, N, 0, nullptr, 0, nullptr, 0, beta, C, ldc);
  return mm(false, true, M, N, K, A, lda, Wm, ldw, beta, C, ldc, nullptr, c.gws, x.gwb, c.hs);
}

// the multi launch's argument table: what is fixed over the steps
MArgs multi_args(const Run &x) {
  const SpGeo &g = x.g;
  MArgs a = {};
  a.B = g.d.B; a.U = g.d.U; a.SE = g.a.SE; a.MU = g.a.MU; a.kind = g.d.kind; a.K = g.d.K; a.F = g.d.F; a.prob_fn = g.d.prob_fn;
  a.dec_len = g.dec_len;
  for (int m = 0; m < g.d.M; ++m) {
    MMem &y = a.m[m];
    y.Te = g.d.Te[m]; y.E = g.d.E[m]; y.coff = g.a.coff[m]; y.S = g.a.S[m];
    y.enc_len = g.enc_len[m]; y.keys = x.r + x.R.keys[m]; y.values = g.values[m]; y.v = g.p.attention_v[m];
    y.ck = g.p.conv_kernel[m]; y.wf = g.p.conv_proj[m];
    y.part = x.w + x.W.part[m];
    y.tickets = reinterpret_cast<unsigned *>(x.w + x.W.tickets) + (size_t)m * g.d.B;
    y.dkeys = x.w + x.W.dkeys[m]; y.dv_part = x.w + x.W.dv[m]; y.dwf_part = x.w + x.W.dwf[m]; y.dck_part = x.w + x.W.dck[m];
    y.dcf_g = x.w + x.W.dcf[m];
  }
  return a;
}

// ===========================================================================
// forward stages

// zero initial state (index 0 of every time-major array) and the decoder inputs actually used (scheduled sampling
// replaces entries of rows 1..L-1 during the steps)
int initial_state(const Run &x) {
  const auto &d = x.g.d;
  const size_t BU = (size_t)d.B * d.U * 4;
  for (int n = 0; n < d.num_layers; ++n) {
    NABU_HIP(hipMemsetAsync(x.r + x.R.H[n], 0, BU, x.s));
    NABU_HIP(hipMemsetAsync(x.r + x.R.Cs[n], 0, BU, x.s));
    if (d.keep_prob < 1.f) NABU_HIP(hipMemsetAsync(x.r + x.R.Ho[n], 0, BU, x.s));
  }
  NABU_HIP(hipMemsetAsync(x.r + x.R.ctx, 0, (size_t)d.B * x.g.a.SE * 4, x.s));
  NABU_HIP(hipMemcpyAsync(x.ids_used(), x.g.ids, (size_t)d.L * d.B * 4, hipMemcpyDeviceToDevice, x.s));
  return 0;
}
// memory m: initial alignment, keys_m = memory_layer_m(values_m)
int memory_keys(const Run &x, int m) {
  const auto &d = x.g.d;
  const int B = d.B, Te = d.Te[m];
  NABU_HIP(hipMemsetAsync(x.r + x.R.align[m], 0, (size_t)B * Te * 4, x.s));
  if (d.kind == 2) NABU_TRY(first_col_one(B, Te, x.r + x.R.align[m], x.s));
  return mm(false, false, B * Te, d.U, d.E[m], x.g.values[m], d.E[m], x.g.p.memory_kernel[m], d.U, 0.f, x.r + x.R.keys[m], d.U,
            nullptr, x.gw, x.gwb, x.s);
}
// multi family: the query kernels side by side, so that q of all mechanisms is one product
int query_columns(const Run &x, int m) {
  if (!x.g.multi) return 0;
  return put_cols(x.g.d.U, x.g.d.U, x.g.p.query_kernel[m], x.w + x.W.wqcat, x.g.a.MU, m * x.g.d.U, x.s);
}
const float *query_weight(const Run &x) { return x.g.multi ? x.w + x.W.wqcat : x.g.p.query_kernel[0]; }
// the dense rows of layer n's kernel (below the embedding rows of layer 0)
const float *dense_rows(const Run &x, int n) { return x.g.p.lstm_kernel[n] + (n == 0 ? (size_t)x.g.d.C * 4 * x.g.d.U : 0); }

int prepare_weights_fwd(const Run &x) {
  const auto &d = x.g.d;
  const int U = d.U, E = x.g.a.SE;
  for (int n = 0; n < d.num_layers; ++n)
    if (x.P.cell_epi[n]) NABU_TRY(permute_gates((n == 0 ? E : U) + U, U, dense_rows(x, n), x.w + x.W.kperm[n], x.s));
  if (x.P.fwd.r16) {
    NABU_TRY(rows16_swizzle_kn(4 * U, E + U, dense_rows(x, 0), 4 * U, x.w + x.W.kxh_sw, U, x.s));
    NABU_TRY(rows16_swizzle_kn(U, U, x.g.p.query_kernel[0], U, x.w + x.W.wq_sw, 0, x.s));
  }
  return 0;
}
int persistent_fwd(const Run &x) {
  const SpGeo &g = x.g;
  const SpReserve &R = x.R;
  float *r = x.r;
  return speller_persist_fwd(x.P.pd, g.dec_len, g.enc_len[0], x.ids_used(), x.w + x.W.kperm[0], g.p.lstm_bias[0],
                             g.p.lstm_kernel[0], g.p.query_kernel[0], g.p.attention_v[0], r + R.keys[0], g.values[0],
                             g.p.conv_kernel[0], g.p.conv_proj[0], r + R.H[0], g.d.keep_prob < 1.f ? r + R.Ho[0] : nullptr,
                             r + R.Cs[0], r + R.acts[0], r + R.q, r + R.ctx, r + R.align[0],
                             reinterpret_cast<int *>(x.w + x.W.status), x.w + x.W.persist, x.P.persist_bytes, x.s, g.p.out_kernel,
                             g.p.out_bias, x.ids_used());
}

// the cell stack of step t: generic (two products + cell kernel) | cell as the product's epilogue | rows16
int cells_fwd(const Run &x, const Chain &c, int t) {
  const auto &d = x.g.d;
  const SpReserve &R = x.R;
  float *r = x.r, *w = x.w;
  const int B = d.B, U = d.U, SE = x.g.a.SE, nl = d.num_layers, Bn = x.P.Bn, b0 = c.b0;
  const bool drop = d.keep_prob < 1.f, r16 = x.P.fwd.r16;
  const size_t cur = (size_t)t * B * U, nxt = (size_t)(t + 1) * B * U;
  float *z = w + x.W.z + (size_t)b0 * 4 * U;
  for (int n = 0; n < nl; ++n) {
    float *Hn = r + R.H[n] + (size_t)b0 * U, *Cn = r + R.Cs[n] + (size_t)b0 * U;
    float *acts = r + R.acts[n] + (size_t)t * B * 4 * U + (size_t)b0 * 4 * U;
    const int K1 = n == 0 ? SE : U;
    const float *x1 = n == 0 ? r + R.ctx + (size_t)t * B * SE + (size_t)b0 * SE : r + R.Ho[n - 1] + nxt + (size_t)b0 * U;
    const float *emb = n == 0 ? x.g.p.lstm_kernel[0] : nullptr;
    const int32_t *ids = n == 0 ? x.ids_used() + (size_t)t * B + b0 : nullptr;
    if (x.P.cell_epi[n]) {   // product + cell in one launch
      SkinnyEpilogue ep = {};
      ep.kind = 1; ep.U = U; ep.step = t; ep.seq_len = c.dlen;
      ep.bias = x.g.p.lstm_bias[n];
      ep.emb = emb; ep.ids = ids;
      ep.c_prev = Cn + cur; ep.h_prev = Hn + cur;
      ep.acts = acts;
      ep.c_new = Cn + nxt; ep.h_new = Hn + nxt;
      const float *Kp = w + x.W.kperm[n];
      if (r16) {
        if (drop) {      // the cell's output dropout in the same launch (the mask of dropout_rows below)
          ep.ho_new = r + R.Ho[n] + nxt + (size_t)b0 * U;
          ep.keep = d.keep_prob; ep.seed = d.seed; ep.seed_offset = d.seed_offset + (unsigned long long)t * nl + n;
          ep.row0 = b0;
        }
        NABU_TRY(rows16(Bn, 4 * U, SE + U, x1, SE, w + x.W.kxh_sw, 0.f, nullptr, 0, c.hs, &ep, nullptr, SE, Hn + cur, U));
      } else {
        NABU_TRY(gemm_skinny_fused(Bn, 4 * U, K1, x1, K1, Kp, 4 * U, U, Hn + cur, U, Kp + (size_t)K1 * 4 * U, 4 * U, 0.f, z,
                                 4 * U, nullptr, w + x.W.fpart + (size_t)c.sub * x.W.fpart_each,
                                 reinterpret_cast<unsigned *>(w + x.W.tickets) + (size_t)c.sub * 1024, c.hs, &ep));
      }
    } else {
      // layer 0: [ctx_0 | .. | ctx_{M-1}] . kernel rows C .. C + sum E — one product on the shared context rows
      const float *Wx = dense_rows(x, n);
      NABU_TRY(mm2(x, c, Bn, 4 * U, K1, x1, K1, Wx, 4 * U, U, Hn + cur, U, Wx + (size_t)K1 * 4 * U, 4 * U, 0.f, z, 4 * U));
      NABU_TRY(nabu_lstm_cell_fwd(Bn, U, t, c.dlen, z, x.g.p.lstm_bias[n], emb, ids, Cn + cur, Hn + cur, acts, Cn + nxt, Hn + nxt,
                                c.hs));
    }
    if (drop && !(r16 && x.P.cell_epi[n]))
      NABU_TRY(dropout_rows((size_t)Bn * U, Hn + nxt, r + R.Ho[n] + nxt + (size_t)b0 * U, d.keep_prob, d.seed,
                          d.seed_offset + (unsigned long long)t * nl + n, (size_t)b0 * U, c.hs));
  }
  return 0;
}
// q_t = h_top . Wq (all mechanisms' queries in one product)
int query_fwd(const Run &x, const Chain &c, const float *htop, float *qt) {
  const int U = x.g.d.U, MU = x.g.a.MU;
  if (x.P.fwd.r16) return rows16(x.P.Bn, U, U, htop, U, x.w + x.W.wq_sw, 0.f, qt, U, c.hs);
  return mm2(x, c, x.P.Bn, MU, U, htop, U, query_weight(x), MU, 0, nullptr, 0, nullptr, 0, 0.f, qt, MU);
}
// the attention step, by entry-point family: a (multi family) carries the launch's table over the steps
int attention_fwd(const Run &x, const Chain &c, int t, const float *qt, MArgs *a) {
  const auto &d = x.g.d;
  const SpReserve &R = x.R;
  float *r = x.r;
  const size_t B = d.B, SE = x.g.a.SE, b0 = c.b0;
  if (x.g.multi) {
    a->step = t; a->q = qt;
    a->ctx_prev = r + R.ctx + t * B * SE;
    a->ctx = r + R.ctx + (t + 1) * B * SE;
    for (int m = 0; m < d.M; ++m) {
      a->m[m].align_prev = r + R.align[m] + t * B * d.Te[m];
      a->m[m].align = r + R.align[m] + (t + 1) * B * d.Te[m];
      a->m[m].znorm = r + R.znorm[m] + t * B;
    }
    return multi_attn_launch(false, x.g.a, *a, c.hs);
  }
  const size_t Te = d.Te[0], E = SE, U = d.U;
  unsigned *atk = x.attn_tickets();
  return attn_fwd_impl(&x.adn, t, c.dlen, x.g.enc_len[0] + b0, r + R.keys[0] + b0 * Te * U, x.g.values[0] + b0 * Te * E, qt,
                       x.g.p.attention_v[0], x.g.p.conv_kernel[0], x.g.p.conv_proj[0], r + R.align[0] + t * B * Te + b0 * Te,
                       r + R.ctx + t * B * E + b0 * E, r + R.align[0] + (t + 1) * B * Te + b0 * Te,
                       r + R.ctx + (t + 1) * B * E + b0 * E, r + R.znorm[0] + t * B + b0,
                       x.w + x.W.attn + (size_t)c.sub * x.W.attn_each, x.attn_fwd_wsb, c.hs, atk ? atk + b0 : nullptr);
}
// ScheduledEmbeddingTrainingHelper: the step's logits decide the next input of selected rows (draws: counter
// (row, sample_offset + t))
int sample_next(const Run &x, const Chain &c, int t, const float *htop) {
  const auto &d = x.g.d;
  const int B = d.B, U = d.U, C = d.C, SE = x.g.a.SE, Bn = x.P.Bn, b0 = c.b0;
  const float *ctx = x.r + x.R.ctx + (size_t)(t + 1) * B * SE + (size_t)b0 * SE;
  const int32_t *teacher = x.g.ids + (size_t)(t + 1) * B + b0;
  int32_t *next = x.ids_used() + (size_t)(t + 1) * B + b0;
  const unsigned long long off = d.sample_offset + (unsigned long long)t;
  if (sample_step_ok(C))     // one launch, logits only for sampled rows
    return sample_step(Bn, C, U, SE, htop, U, ctx, SE, x.g.p.out_kernel, x.g.p.out_bias, d.sample_prob, d.sample_seed, off, teacher,
                       next, b0, c.hs);
  float *lt = x.r + x.R.logits_tm + (size_t)t * B * C + (size_t)b0 * C;
  NABU_TRY(mm(false, false, Bn, C, U, htop, U, x.g.p.out_kernel, C, 0.f, lt, C, x.g.p.out_bias, c.gws, x.gwb, c.hs));
  NABU_TRY(mm(false, false, Bn, C, SE, ctx, SE, x.g.p.out_kernel + (size_t)U * C, C, 1.f, lt, C, nullptr, c.gws, x.gwb, c.hs));
  return sample_ids_rows(Bn, C, lt, d.sample_prob, d.sample_seed, off, teacher, next, b0, c.hs);
}
// all steps of one chain
int steps_fwd(const Run &x, int sub) {
  const auto &d = x.g.d;
  const Chain c = chain_of(x, sub);
  const int B = d.B, U = d.U, MU = x.g.a.MU, L = d.L;
  MArgs a;
  if (x.g.multi) a = multi_args(x);
  for (int t = 0; t < L; ++t) {
    NABU_TRY(cells_fwd(x, c, t));
    const float *htop = x.r + x.R.Ho[d.num_layers - 1] + (size_t)(t + 1) * B * U + (size_t)c.b0 * U;
    float *qt = x.r + x.R.q + (size_t)t * B * MU + (size_t)c.b0 * MU;
    NABU_TRY(query_fwd(x, c, htop, qt));
    NABU_TRY(attention_fwd(x, c, t, qt, &a));
    if (d.sample_prob > 0.f && t + 1 < L) NABU_TRY(sample_next(x, c, t, htop));
  }
  return 0;
}
// the step chain: fork the sub-batch streams, enqueue every chain, join.  The side streams are joined before an
// error is propagated: chains already enqueued must not outlive the call
template <typename F>
int step_chain(Run &x, F steps) {
  NABU_TRY(sub_streams(x.P.NS, x.s, &x.ss));
  NABU_TRY(sub_fork(x.ss));
  const Run &cx = x;
  const int e_run = run_subs(x.P.NS, x.P.threads, [&](int sub) { return steps(cx, sub); }), e_join = sub_join(x.ss);
  return e_run ? e_run : e_join;
}
// output projection of all steps: [h_t | contexts_t] · W + b, then batch-major + impute_finished
int project_fwd(const Run &x, float *logits) {
  const auto &d = x.g.d;
  const int B = d.B, L = d.L, U = d.U, C = d.C, SE = x.g.a.SE;
  float *ltm = x.r + x.R.logits_tm;
  NABU_TRY(mm(false, false, L * B, C, U, x.r + x.R.Ho[d.num_layers - 1] + (size_t)B * U, U, x.g.p.out_kernel, C, 0.f, ltm, C,
            x.g.p.out_bias, x.gw, x.gwb, x.s));
  NABU_TRY(mm(false, false, L * B, C, SE, x.r + x.R.ctx + (size_t)B * SE, SE, x.g.p.out_kernel + (size_t)U * C, C, 1.f, ltm, C,
            nullptr, x.gw, x.gwb, x.s));
  NABU_TRY(nabu_swap01_f32(L, B, C, ltm, logits, x.s));
  return nabu_mask_time_f32(B, L, C, logits, x.g.dec_len, x.s);
}

int speller_forward(const SpGeo &g, float *logits, void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream,
                    const char *who) {
  Run x = {g};
  NABU_TRY(make_run(g, reserve, ws, ws_bytes, stream, who, &x));
  NABU_HIP(hipMemsetAsync(x.w + x.W.tickets, 0, x.W.tickets_n * 4, x.s));
  NABU_TRY(initial_state(x));
  for (int m = 0; m < g.d.M; ++m) {
    NABU_TRY(memory_keys(x, m));
    NABU_TRY(query_columns(x, m));
  }
  NABU_TRY(prepare_weights_fwd(x));
  if (x.P.fwd.persist) NABU_TRY(persistent_fwd(x));
  else NABU_TRY(step_chain(x, steps_fwd));
  return project_fwd(x, logits);
}

// ===========================================================================
// backward stages

// output projection: d out_kernel, d out_bias; dH [L,B,U] and dCtx [L,B,sum E] start as its shares
int project_bwd(const Run &x, const float *dlogits) {
  const auto &d = x.g.d;
  const int B = d.B, L = d.L, U = d.U, C = d.C, SE = x.g.a.SE, BL = B * L;
  float *dl = x.w + x.W.dl, *gw = x.gw;
  const size_t gwb = x.gwb;
  const float *htop_all = x.r + x.R.Ho[d.num_layers - 1] + (size_t)B * U;   // h_top[t], t = 0..L-1
  const float *ctx1 = x.r + x.R.ctx + (size_t)B * SE;                        // ctx[t]
  NABU_TRY(nabu_swap01_f32(B, L, C, dlogits, dl, x.s));      // [B,L,C] -> [L,B,C]
  NABU_TRY(mm(true, false, U, C, BL, htop_all, U, dl, C, 0.f, x.g.gr.out_kernel, C, nullptr, gw, gwb, x.s));
  NABU_TRY(mm(true, false, SE, C, BL, ctx1, SE, dl, C, 0.f, x.g.gr.out_kernel + (size_t)U * C, C, nullptr, gw, gwb, x.s));
  NABU_TRY(nabu_colsum_f32(BL, C, dl, C, 0.f, x.g.gr.out_bias, gw, gwb, x.s));
  NABU_TRY(mm(false, true, BL, U, C, dl, C, x.g.p.out_kernel, C, 0.f, x.w + x.W.dH, U, nullptr, gw, gwb, x.s));
  return mm(false, true, BL, SE, C, dl, C, x.g.p.out_kernel + (size_t)U * C, C, 0.f, x.w + x.W.dCtx, SE, nullptr, gw, gwb, x.s);
}
// zero carries of the last step and the accumulators of the attention launches
int zero_accumulators(const Run &x) {
  const auto &d = x.g.d;
  const size_t B = d.B, U = d.U;
  NABU_HIP(hipMemsetAsync(x.w + x.W.tickets, 0, x.W.tickets_n * 4, x.s));
  for (int n = 0; n < d.num_layers; ++n) {
    NABU_HIP(hipMemsetAsync(x.w + x.W.dh[0][n], 0, B * U * 4, x.s));
    NABU_HIP(hipMemsetAsync(x.w + x.W.dc[0][n], 0, B * U * 4, x.s));
  }
  for (int m = 0; m < d.M; ++m) {
    const size_t S = x.g.multi ? x.g.a.S[m] : x.P.S;
    NABU_HIP(hipMemsetAsync(x.w + x.W.dkeys[m], 0, B * d.Te[m] * U * 4, x.s));
    NABU_HIP(hipMemsetAsync(x.w + x.W.dv[m], 0, B * S * U * 4, x.s));
    if (d.kind == 1) {
      NABU_HIP(hipMemsetAsync(x.w + x.W.dwf[m], 0, B * S * d.F * U * 4, x.s));
      NABU_HIP(hipMemsetAsync(x.w + x.W.dck[m], 0, B * d.K * d.F * 4, x.s));
    }
    NABU_TRY(query_columns(x, m));
  }
  return 0;
}
int prepare_weights_bwd(const Run &x) {
  const auto &d = x.g.d;
  const int U = d.U, E = x.g.a.SE;
  float *w = x.w;
  if (x.P.weights_T) {
    // transposed copies of the weights the per-step gradient products use: dz·W^T becomes a row-major product
    // with M = B rows, which the skinny GEMM kernel streams in a few microseconds
    NABU_TRY(transpose(U, U, x.g.p.query_kernel[0], U, w + x.W.wqT, x.s));
    for (int n = 0; n < d.num_layers; ++n) {
      const int K1 = n == 0 ? E : U;
      NABU_TRY(transpose(K1, 4 * U, dense_rows(x, n), 4 * U, w + x.W.kxT[n], x.s));
      NABU_TRY(transpose(U, 4 * U, dense_rows(x, n) + (size_t)K1 * 4 * U, 4 * U, w + x.W.khT[n], x.s));
    }
  }
  if (x.P.fuse_b) NABU_TRY(transpose(E + U, 4 * U, dense_rows(x, 0), 4 * U, w + x.W.kxhT, x.s));
  if (x.P.bwd.r16) {
    NABU_TRY(rows16_swizzle(U, U, x.g.p.query_kernel[0], U, w + x.W.wq_sw, x.s));
    NABU_TRY(rows16_swizzle(E + U, 4 * U, dense_rows(x, 0), 4 * U, w + x.W.kxh_sw, x.s));
  }
  return 0;
}
// (output dropout is applied inside the kernel: the scale factors are drawn again from the Philox stream by a small
// launch in front of it)
int persistent_bwd(const Run &x) {
  const SpGeo &g = x.g;
  const SpReserve &R = x.R;
  const SpWs &W = x.W;
  float *r = x.r, *w = x.w;
  const bool loc = g.d.kind == 1;
  return speller_persist_bwd(x.P.pd_bwd, g.dec_len, g.enc_len[0], w + W.kxhT, g.p.query_kernel[0], g.p.attention_v[0],
                             r + R.keys[0], g.values[0], r + R.acts[0], r + R.Cs[0], r + R.q, r + R.ctx, r + R.align[0],
                             w + W.dH, w + W.dCtx, w + W.dq, w + W.dz[0], w + W.dkeys[0], w + W.dv8,
                             reinterpret_cast<int *>(w + W.status), w + W.persist, x.P.persist_bytes, x.s, g.p.conv_kernel[0],
                             g.p.conv_proj[0], w + W.ds_all, loc ? w + W.cf_all : nullptr, loc ? w + W.dck8 : nullptr);
}

// the carries of a chain between its steps
struct Carry {
  int cur = 0;            // index of the dh / dc carries coming from step t + 1
  bool have = false;
};
// d context carried from step t + 1 joins the output projection's share in dCt (the split product has put it there)
int carry_context(const Run &x, const Chain &c, int t, const Carry &k, float *dCt) {
  if (!k.have || x.P.split_b) return 0;
  const int SE = x.g.a.SE, U = x.g.d.U, Bn = x.P.Bn;
  if (x.P.fuse_b)
    return add_rows(Bn, SE, x.w + x.W.dxh[(t + 1) & 1] + (size_t)c.b0 * (SE + U), SE + U, dCt, SE, c.hs);
  return nabu_axpy_f32((size_t)Bn * SE, 1.f, x.w + x.W.dctx[(t + 1) & 1] + (size_t)c.b0 * SE, dCt, c.hs);
}
int attention_bwd(const Run &x, const Chain &c, int t, const Carry &k, const float *dCt, float *dqt, MArgs *a) {
  const auto &d = x.g.d;
  const SpReserve &R = x.R;
  const SpWs &W = x.W;
  float *r = x.r, *w = x.w;
  const size_t B = d.B, SE = x.g.a.SE, b0 = c.b0;
  const bool loc = d.kind == 1;
  if (x.g.multi) {
    a->step = t; a->q = r + R.q + t * B * x.g.a.MU;
    a->ctx = r + R.ctx + (t + 1) * B * SE;
    a->dctx = dCt; a->dq = dqt;
    for (int m = 0; m < d.M; ++m) {
      MMem &y = a->m[m];
      y.align_prev = r + R.align[m] + t * B * d.Te[m];
      y.align_c = r + R.align[m] + (t + 1) * B * d.Te[m];
      y.znorm = r + R.znorm[m] + t * B;
      y.dalign_out = loc ? w + W.dal[t & 1][m] : nullptr;
      y.dalign_in = (loc && k.have) ? w + W.dal[(t + 1) & 1][m] : nullptr;
    }
    return multi_attn_launch(true, x.g.a, *a, c.hs);
  }
  const size_t Te = d.Te[0], E = SE, U = d.U, S = x.P.S, F = d.F, K = d.K;
  unsigned *atk = x.attn_tickets();
  const bool defer = x.P.Sp > 0;
  return attn_bwd_impl(&x.adn, t, c.dlen, x.g.enc_len[0] + b0, r + R.keys[0] + b0 * Te * U, x.g.values[0] + b0 * Te * E,
                       r + R.q + t * B * U + b0 * U, x.g.p.attention_v[0], x.g.p.conv_kernel[0], x.g.p.conv_proj[0],
                       r + R.align[0] + t * B * Te + b0 * Te, r + R.align[0] + (t + 1) * B * Te + b0 * Te,
                       r + R.ctx + (t + 1) * B * E + b0 * E, dCt, (loc && k.have) ? w + W.dal[(t + 1) & 1][0] + b0 * Te : nullptr,
                       dqt, w + W.dkeys[0] + b0 * Te * U, w + W.dv[0] + b0 * S * U, loc ? w + W.dwf[0] + b0 * S * F * U : nullptr,
                       loc ? w + W.dck[0] + b0 * K * F : nullptr, loc ? w + W.dal[t & 1][0] + b0 * Te : nullptr,
                       r + R.znorm[0] + t * B + b0, w + W.attn + (size_t)c.sub * W.attn_each, x.attn_bwd_wsb, c.hs,
                       atk ? atk + b0 : nullptr, defer ? w + W.ds_all + (t * B + b0) * Te : nullptr,
                       (defer && loc) ? w + W.cf_all + (t * B + b0) * Te * F : nullptr);
}
// the single-layer cell of step t as the epilogue of dq·Wq^T, then ONE dz·[Kx^T | Kh^T] product: gemm_skinny_fused | rows16
int cells_bwd_fused(const Run &x, const Chain &c, int t, const Carry &k, const float *dqt, float *dHt) {
  const auto &d = x.g.d;
  const SpWs &W = x.W;
  float *r = x.r, *w = x.w;
  const int B = d.B, U = d.U, E = x.g.a.SE, Bn = x.P.Bn, b0 = c.b0;
  float *dzt = w + W.dz[0] + (size_t)t * B * 4 * U + (size_t)b0 * 4 * U;
  const float *Cn = r + x.R.Cs[0] + (size_t)b0 * U;
  float *dCprev = t > 0 ? w + W.dCtx + (size_t)(t - 1) * B * E + (size_t)b0 * E : nullptr;
  float *dxh = w + W.dxh[t & 1] + (size_t)b0 * (E + U);
  SkinnyEpilogue ep = {};
  ep.kind = 2; ep.U = U; ep.step = t; ep.seq_len = c.dlen;
  ep.acts = r + x.R.acts[0] + (size_t)t * B * 4 * U + (size_t)b0 * 4 * U;
  ep.c_new = const_cast<float *>(Cn + (size_t)(t + 1) * B * U);
  ep.c_prev = Cn + (size_t)t * B * U;
  ep.dh2 = k.have ? w + W.dxh[(t + 1) & 1] + (size_t)b0 * (E + U) + E : nullptr;
  ep.ld_dh2 = E + U;
  ep.dc_in = w + W.dc[k.cur][0] + (size_t)b0 * U;
  ep.dz = dzt;
  ep.dc_out = w + W.dc[k.cur ^ 1][0] + (size_t)b0 * U;
  ep.keep = d.keep_prob < 1.f ? d.keep_prob : 1.f; ep.seed = d.seed; ep.seed_offset = d.seed_offset + (unsigned long long)t;
  ep.row0 = b0;
  // d context of step t-1 goes straight into that step's dCtx row block (on top of the output projection's
  // share), d h into the carry: no separate add launch in front of the next attention
  SkinnySplit sp = {dxh + E, E + U, E, 0.f};
  if (x.P.bwd.r16) {
    NABU_TRY(rows16(Bn, U, U, dqt, U, w + W.wq_sw, 1.f, dHt, U, c.hs, &ep));
    if (t > 0) NABU_TRY(rows16(Bn, E + U, 4 * U, dzt, 4 * U, w + W.kxh_sw, 1.f, dCprev, E, c.hs, nullptr, &sp));
    return 0;
  }
  float *fp = w + W.fpart + (size_t)c.sub * W.fpart_each;
  unsigned *tk = reinterpret_cast<unsigned *>(w + W.tickets) + (size_t)c.sub * 1024;
  NABU_TRY(gemm_skinny_fused(Bn, U, U, dqt, U, w + W.wqT, U, 0, nullptr, 0, nullptr, 0, 1.f, dHt, U, nullptr, fp, tk, c.hs, &ep));
  if (x.P.split_b && t > 0)
    return gemm_skinny_fused(Bn, E + U, 4 * U, dzt, 4 * U, w + W.kxhT, E + U, 0, nullptr, 0, nullptr, 0, 1.f, dCprev, E, nullptr,
                             fp, tk, c.hs, nullptr, &sp);
  return gemm_skinny_fused(Bn, E + U, 4 * U, dzt, 4 * U, w + W.kxhT, E + U, 0, nullptr, 0, nullptr, 0, 0.f, dxh, E + U, nullptr, fp,
                           tk, c.hs, nullptr);
}
// the generic cell stack of step t: d h_top += dq · Wq^T, then per layer (dropout,) cell kernel and the two products
int cells_bwd(const Run &x, const Chain &c, int t, const Carry &k, const float *dqt, float *dHt) {
  const auto &d = x.g.d;
  const SpWs &W = x.W;
  float *r = x.r, *w = x.w;
  const int B = d.B, U = d.U, SE = x.g.a.SE, MU = x.g.a.MU, nl = d.num_layers, Bn = x.P.Bn, b0 = c.b0, cur = k.cur;
  NABU_TRY(mmT(x, c, Bn, U, MU, dqt, MU, w + W.wqT, query_weight(x), MU, 1.f, dHt, U));
  const float *dtop = dHt;
  for (int n = nl - 1; n >= 0; --n) {
    const float *dh_in = dtop;
    if (d.keep_prob < 1.f) {
      NABU_TRY(dropout_rows((size_t)Bn * U, dtop, w + W.tmp + (size_t)b0 * U, d.keep_prob, d.seed,
                          d.seed_offset + (unsigned long long)t * nl + n, (size_t)b0 * U, c.hs));
      dh_in = w + W.tmp + (size_t)b0 * U;
    }
    float *dzt = w + W.dz[n] + (size_t)t * B * 4 * U + (size_t)b0 * 4 * U;
    const float *Cn = r + x.R.Cs[n] + (size_t)b0 * U;
    NABU_TRY(nabu_lstm_cell_bwd(Bn, U, t, c.dlen, r + x.R.acts[n] + (size_t)t * B * 4 * U + (size_t)b0 * 4 * U,
                              Cn + (size_t)(t + 1) * B * U, Cn + (size_t)t * B * U, dh_in, w + W.dh[cur][n] + (size_t)b0 * U,
                              w + W.dc[cur][n] + (size_t)b0 * U, dzt, w + W.dc[cur ^ 1][n] + (size_t)b0 * U, c.hs));
    // d (layer input) and d h_(t-1): layer 0's input gradient is d context, carried to step t - 1
    const int K1 = n == 0 ? SE : U;
    float *dx = n == 0 ? w + W.dctx[t & 1] + (size_t)b0 * SE : w + W.dx + (size_t)b0 * U;
    const float *Wx = dense_rows(x, n);
    NABU_TRY(mmT(x, c, Bn, K1, 4 * U, dzt, 4 * U, w + W.kxT[n], Wx, 4 * U, 0.f, dx, K1));
    NABU_TRY(mmT(x, c, Bn, U, 4 * U, dzt, 4 * U, w + W.khT[n], Wx + (size_t)K1 * 4 * U, 4 * U, 0.f,
               w + W.dh[cur ^ 1][n] + (size_t)b0 * U, U));
    dtop = dx;
  }
  return 0;
}
int steps_bwd(const Run &x, int sub) {
  const auto &d = x.g.d;
  const Chain c = chain_of(x, sub);
  const size_t B = d.B, U = d.U, SE = x.g.a.SE, MU = x.g.a.MU;
  MArgs a;
  if (x.g.multi) a = multi_args(x);
  Carry k;
  for (int t = d.L - 1; t >= 0; --t) {
    float *dCt = x.w + x.W.dCtx + t * B * SE + c.b0 * SE;
    float *dqt = x.w + x.W.dq + t * B * MU + c.b0 * MU;
    float *dHt = x.w + x.W.dH + t * B * U + c.b0 * U;
    NABU_TRY(carry_context(x, c, t, k, dCt));
    NABU_TRY(attention_bwd(x, c, t, k, dCt, dqt, &a));
    if (x.P.fuse_b) NABU_TRY(cells_bwd_fused(x, c, t, k, dqt, dHt));
    else NABU_TRY(cells_bwd(x, c, t, k, dqt, dHt));
    k.have = true;
    k.cur ^= 1;
  }
  return 0;
}
// d keys / d attention_v / d conv_proj of all steps in ONE launch after the steps (attn_param_grads_kernel)
int deferred_attention_grads(const Run &x) {
  const SpGeo &g = x.g;
  const nabu_attn_desc adb = attn_desc(g, 0, g.d.B);
  return attn_param_grads(&adb, x.P.Sp, g.d.L, g.dec_len, g.enc_len[0], x.r + x.R.keys[0], x.r + x.R.q, g.p.attention_v[0],
                          g.p.conv_proj[0], x.w + x.W.ds_all, x.w + x.W.cf_all, x.w + x.W.dkeys[0], x.w + x.W.dv16,
                          x.w + x.W.dwf16, x.s);
}
// weight gradients that are sums over steps, as single products over all steps
int sums_over_steps(const Run &x) {
  const auto &d = x.g.d;
  const int B = d.B, U = d.U, C = d.C, SE = x.g.a.SE, MU = x.g.a.MU, BL = B * d.L;
  float *r = x.r, *gw = x.gw;
  const size_t gwb = x.gwb;
  const float *htop_all = r + x.R.Ho[d.num_layers - 1] + (size_t)B * U;
  for (int m = 0; m < d.M; ++m)
    NABU_TRY(mm(true, false, U, U, BL, htop_all, U, x.w + x.W.dq + (size_t)m * U, MU, 0.f, x.g.gr.query_kernel[m], U, nullptr, gw,
              gwb, x.s));
  for (int n = 0; n < d.num_layers; ++n) {
    const float *dzn = x.w + x.W.dz[n];
    float *gK = x.g.gr.lstm_kernel[n];
    const int K1 = n == 0 ? SE : U;
    const float *x1 = n == 0 ? r + x.R.ctx : r + x.R.Ho[n - 1] + (size_t)B * U;
    if (n == 0) {
      NABU_TRY(nabu_scatter_rows_f32(C, BL, 4 * U, reinterpret_cast<const int32_t *>(r + x.R.ids), dzn, gK, x.s));
      gK += (size_t)C * 4 * U;
    }
    NABU_TRY(mm(true, false, K1, 4 * U, BL, x1, K1, dzn, 4 * U, 0.f, gK, 4 * U, nullptr, gw, gwb, x.s));
    NABU_TRY(mm(true, false, U, 4 * U, BL, r + x.R.H[n], U, dzn, 4 * U, 0.f, gK + (size_t)K1 * 4 * U, 4 * U, nullptr, gw, gwb, x.s));
    NABU_TRY(nabu_colsum_f32(BL, 4 * U, dzn, 4 * U, 0.f, x.g.gr.lstm_bias[n], gw, gwb, x.s));
  }
  return 0;
}
// attention_v / conv_proj / conv_kernel of memory m: column sums of the partial rows, by their source — the
// persistent kernel's | the deferred launch's | the per-step launches' (one row per utterance and frame slice)
int attention_param_sums(const Run &x, int m) {
  const auto &d = x.g.d;
  const SpWs &W = x.W;
  const int B = d.B, U = d.U, F = d.F, K = d.K, S = x.g.multi ? x.g.a.S[m] : x.P.S, Sp = x.P.Sp;
  const bool persist = x.P.bwd.persist, defer = Sp > 0;
  float *w = x.w, *gw = x.gw;
  const size_t gwb = x.gwb;
  const nabu_speller_multi_grads &gr = x.g.gr;
  if (persist && !defer) NABU_TRY(nabu_colsum_f32(B * 8, U, w + W.dv8, U, 0.f, gr.attention_v[m], gw, gwb, x.s));
  else if (defer)        NABU_TRY(nabu_colsum_f32(B * Sp, U, w + W.dv16, U, 0.f, gr.attention_v[m], gw, gwb, x.s));
  else                   NABU_TRY(nabu_colsum_f32(B * S, U, w + W.dv[m], U, 0.f, gr.attention_v[m], gw, gwb, x.s));
  if (d.kind != 1) return 0;
  if (defer) NABU_TRY(nabu_colsum_f32(B * Sp, F * U, w + W.dwf16, F * U, 0.f, gr.conv_proj[m], gw, gwb, x.s));
  else       NABU_TRY(nabu_colsum_f32(B * S, F * U, w + W.dwf[m], F * U, 0.f, gr.conv_proj[m], gw, gwb, x.s));
  if (persist) return nabu_colsum_f32(B * 8, K * F, w + W.dck8, K * F, 0.f, gr.conv_kernel[m], gw, gwb, x.s);
  return nabu_colsum_f32(B, K * F, w + W.dck[m], K * F, 0.f, gr.conv_kernel[m], gw, gwb, x.s);
}
// keys_m = values_m · Wmem_m ; context_t = align_t^T · values_m
int memory_grads(const Run &x, int m) {
  const auto &d = x.g.d;
  const int B = d.B, U = d.U, Te = d.Te[m], E = d.E[m], SE = x.g.a.SE;
  const float *dkeys = x.w + x.W.dkeys[m];
  float *dvalues = x.g.dvalues[m];
  NABU_TRY(mm(true, false, E, U, B * Te, x.g.values[m], E, dkeys, U, 0.f, x.g.gr.memory_kernel[m], U, nullptr, x.gw, x.gwb, x.s));
  NABU_TRY(mm(false, true, B * Te, E, U, dkeys, U, x.g.p.memory_kernel[m], U, 0.f, dvalues, E, nullptr, x.gw, x.gwb, x.s));
  // dvalues_m[b] += align_m[:, b, :]^T · dCtx[:, b, columns of m] for every utterance: one batched launch
  return gemm_batched_f32(true, false, Te, E, d.L, x.r + x.R.align[m] + (size_t)B * Te, B * Te, Te,
                          x.w + x.W.dCtx + x.g.a.coff[m], B * SE, SE, 1.f, dvalues, E, (long long)Te * E, B, x.s);
}

int speller_backward(const SpGeo &g, const float *dlogits, void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream,
                     const char *who) {
  Run x = {g};
  NABU_TRY(make_run(g, reserve, ws, ws_bytes, stream, who, &x));
  NABU_TRY(project_bwd(x, dlogits));
  NABU_TRY(zero_accumulators(x));
  NABU_TRY(prepare_weights_bwd(x));
  if (x.P.bwd.persist) NABU_TRY(persistent_bwd(x));
  else NABU_TRY(step_chain(x, steps_bwd));
  if (x.P.Sp > 0) NABU_TRY(deferred_attention_grads(x));
  NABU_TRY(sums_over_steps(x));
  for (int m = 0; m < g.d.M; ++m) {
    NABU_TRY(attention_param_sums(x, m));
    NABU_TRY(memory_grads(x, m));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// the queries
size_t reserve_bytes(const SpGeo &g) { return sp_reserve(g).total * sizeof(float); }
size_t ws_bytes_of(const SpGeo &g) { return sp_ws(g, speller_plan(g, nullptr)).total * sizeof(float); }
int decoder_inputs(const SpGeo &g, const void *reserve, int32_t *out_ids, nabu_stream_t stream) {
  NABU_HIP(hipMemcpyAsync(out_ids, static_cast<const float *>(reserve) + sp_reserve(g).ids, (size_t)g.d.L * g.d.B * 4,
                          hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return 0;
}

}  // namespace

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_speller_reserve_bytes(const nabu_speller_desc *d) {
  SpGeo g;
  return geo_of(d, &g) ? 0 : reserve_bytes(g);
}
extern "C" size_t nabu_speller_ws_bytes(const nabu_speller_desc *d) {
  SpGeo g;
  return geo_of(d, &g) ? 0 : ws_bytes_of(g);
}
extern "C" int nabu_speller_uses_persistent(const nabu_speller_desc *d, int backward) {
  SpGeo g;
  if (geo_of(d, &g)) return 0;
  const SpellerPlan P = speller_plan(g, nullptr);
  return (backward ? P.bwd.persist : P.fwd.persist) ? 1 : 0;
}
extern "C" int nabu_speller_decoder_inputs(const nabu_speller_desc *d, const void *reserve, int32_t *out_ids,
                                           nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(reserve && out_ids, "speller_decoder_inputs: null pointer");
  return decoder_inputs(g, reserve, out_ids, stream);
}
extern "C" int nabu_speller_fwd(const nabu_speller_desc *d, const float *values, const int32_t *enc_len,
                                const int32_t *ids, const int32_t *dec_len, const nabu_speller_params *p,
                                float *logits, void *reserve, void *ws, size_t ws_bytes,
                                nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(values && enc_len && ids && dec_len && p && logits && reserve && ws, "speller_fwd: null pointer");
  operands(&g, values, enc_len, ids, dec_len, p, nullptr, nullptr);
  return speller_forward(g, logits, reserve, ws, ws_bytes, stream, "speller_fwd");
}
extern "C" int nabu_speller_bwd(const nabu_speller_desc *d, const float *values, const int32_t *enc_len,
                                const int32_t *ids, const int32_t *dec_len, const nabu_speller_params *p,
                                const float *dlogits, void *reserve, const nabu_speller_grads *gr,
                                float *dvalues, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(values && enc_len && ids && dec_len && p && dlogits && reserve && gr && dvalues && ws,
                 "speller_bwd: null pointer");
  operands(&g, values, enc_len, ids, dec_len, p, gr, dvalues);
  return speller_backward(g, dlogits, reserve, ws, ws_bytes, stream, "speller_bwd");
}

extern "C" size_t nabu_speller_multi_reserve_bytes(const nabu_speller_multi_desc *d) {
  SpGeo g;
  return geo_of(d, &g) ? 0 : reserve_bytes(g);
}
extern "C" size_t nabu_speller_multi_ws_bytes(const nabu_speller_multi_desc *d) {
  SpGeo g;
  return geo_of(d, &g) ? 0 : ws_bytes_of(g);
}
extern "C" int nabu_speller_multi_uses_persistent(const nabu_speller_multi_desc *d, int backward) {
  SpGeo g;
  if (geo_of(d, &g)) return 0;
  const SpellerPlan P = speller_plan(g, nullptr);
  return (backward ? P.bwd.persist : P.fwd.persist) ? 1 : 0;
}
extern "C" int nabu_speller_multi_attn_slices(const nabu_speller_multi_desc *d, int m) {
  SpGeo g;
  if (geo_of(d, &g) || m < 0 || m >= d->M) return 0;
  return g.a.S[m];
}
extern "C" int nabu_speller_multi_decoder_inputs(const nabu_speller_multi_desc *d, const void *reserve, int32_t *out_ids,
                                                 nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(reserve && out_ids, "speller_multi_decoder_inputs: null pointer");
  return decoder_inputs(g, reserve, out_ids, stream);
}
extern "C" int nabu_speller_multi_fwd(const nabu_speller_multi_desc *d, const float *const *values,
                                      const int32_t *const *enc_len, const int32_t *ids, const int32_t *dec_len,
                                      const nabu_speller_multi_params *p, float *logits, void *reserve, void *ws,
                                      size_t ws_bytes, nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(values && enc_len && ids && dec_len && p && logits && reserve && ws, "speller_multi_fwd: null pointer");
  NABU_TRY(operands(&g, values, enc_len, ids, dec_len, p, nullptr, nullptr));
  return speller_forward(g, logits, reserve, ws, ws_bytes, stream, "speller_multi_fwd");
}
extern "C" int nabu_speller_multi_bwd(const nabu_speller_multi_desc *d, const float *const *values,
                                      const int32_t *const *enc_len, const int32_t *ids, const int32_t *dec_len,
                                      const nabu_speller_multi_params *p, const float *dlogits, void *reserve,
                                      const nabu_speller_multi_grads *gr, float *const *dvalues, void *ws,
                                      size_t ws_bytes, nabu_stream_t stream) {
  SpGeo g;
  if (int e = geo_of(d, &g)) return e;
  NABU_CHECK_ARG(values && enc_len && ids && dec_len && p && dlogits && reserve && gr && dvalues && ws,
                 "speller_multi_bwd: null pointer");
  NABU_TRY(operands(&g, values, enc_len, ids, dec_len, p, gr, dvalues));
  return speller_backward(g, dlogits, reserve, ws, ws_bytes, stream, "speller_multi_bwd");
}
