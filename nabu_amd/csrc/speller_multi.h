// speller_multi.h — the multi-mechanism attention launches of speller_multi.hip for the drivers outside that file
// (decode.hip: the beam search; speller_train.hip: the training driver).
#pragma once
#include "common.h"

namespace nabu {

struct MultiAttnMem {
  int Te, E;
  const int32_t *enc_len;
  const float *keys, *values, *v, *ck, *wf, *align_prev;
  float *align, *znorm;
  float *part;        // [B, S, E + 4] floats, S = nabu_attn_bwd_slices of (B, Te, E, U, ...): multi_attn_part_floats
  unsigned *tickets;  // [B] zeroed counters (left zero)
};
size_t multi_attn_part_floats(int B, int Te, int E, int U, int kind, int K, int F, int prob_fn);
// ONE launch for the M mechanisms of a step: q [B, M U], ctx_prev / ctx [B, sum E] (mechanism m at the offset of
// the E of the mechanisms before it); semantics per mechanism: nabu_attn_fwd
int multi_attn_fwd(int M, int B, int U, int kind, int K, int F, int prob_fn, int step, const int32_t *dec_len, const float *q,
                   const float *ctx_prev, float *ctx, const MultiAttnMem *mems, hipStream_t s);
// dst[r, c0 + c] = src[r, c] for an [R, Cn] src: the query kernels side by side in the [U, M U] operand of q
int put_cols(int R, int Cn, const float *src, float *dst, int ldd, int c0, hipStream_t s);


// ---- the training driver's access: the launch's own argument table, filled by the caller once per call and per step
// one mechanism of a launch
struct MMem {
  int Te, E, coff, S;            // encoder frames, encoder dim, column offset in the [B, sum E] buffers, frame slices
  const int32_t *enc_len;
  const float *keys, *values, *v, *ck, *wf;
  const float *align_prev, *align_c;   // [B,Te]: previous alignment; this step's alignment (backward)
  float *align;                  // forward output
  float *znorm;                  // [B] normaliser of normalized_sigmoid
  float *part;                   // forward: [B,S,E+4] partial context + (local max, local sum); backward: [B,S,U] dq
  unsigned *tickets;             // [B] zeroed counters (left zero)
  // backward
  const float *dalign_in;
  float *dalign_out, *dkeys, *dv_part, *dwf_part, *dck_part, *dcf_g;
};
struct MArgs {
  int B, U, SE, MU, kind, K, F, step, prob_fn;
  const int32_t *dec_len;
  const float *q;                // [B, M U]
  const float *ctx_prev;         // [B, sum E]
  float *ctx;                    // [B, sum E] (backward: this step's contexts, read only)
  const float *dctx;             // [B, sum E]
  float *dq;                     // [B, M U]
  MMem m[NABU_SPELLER_MAX_MEMORIES];
};
// what a launch over the M memories of a descriptor needs: column offsets in the [B, sum E] buffers, frame slices
// per memory (nabu_attn_bwd_slices), dynamic LDS of either pass
struct MultiAttnGeo {
  int M, SE, MU, S[NABU_SPELLER_MAX_MEMORIES], Smax, coff[NABU_SPELLER_MAX_MEMORIES];
  size_t lds_f, lds_b;
};
// checks the descriptor (NABU_E* with the error text set) and fills g
int multi_attn_geo(const nabu_speller_multi_desc *d, MultiAttnGeo *g);
// attn_multi_fwd_kernel / attn_multi_bwd_kernel<a.kind == 1>, grid (B, Smax, M)
int multi_attn_launch(bool backward, const MultiAttnGeo &g, const MArgs &a, hipStream_t s);

}  // namespace nabu
