// speller_multi.h — the multi-mechanism attention forward launch of speller_multi.hip for the drivers outside that
// file (decode.hip: the beam search).
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

}  // namespace nabu
