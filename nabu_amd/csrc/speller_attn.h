// speller_attn.h — what speller.hip (cell, attention and utility kernels of the one-memory decoder) offers to the
// training driver (speller_train.hip).  Semantics of the attention calls: nabu_attn_fwd / nabu_attn_bwd.
#pragma once
#include "common.h"

namespace nabu {

int check_attn(const nabu_attn_desc *d);
// frame slices per utterance of the attention launches (1 for batches that fill the chip)
int attn_bwd_nslices(const nabu_attn_desc *d);
// tickets: B zeroed counters (left zero) -> the finish steps run inside the attention launches
int attn_fwd_impl(const nabu_attn_desc *d, int step, const int32_t *dec_len, const int32_t *enc_len, const float *keys,
                  const float *values, const float *q, const float *v, const float *conv_kernel, const float *conv_proj,
                  const float *align_prev, const float *ctx_prev, float *align, float *ctx, float *znorm, void *ws,
                  size_t ws_bytes, nabu_stream_t stream, unsigned *tickets);
// ds_out / cf_out given: d keys / d attention_v / d conv_proj are NOT accumulated; the step's d scores and location
// features are left for attn_param_grads, one launch after the last step
int attn_bwd_impl(const nabu_attn_desc *d, int step, const int32_t *dec_len, const int32_t *enc_len, const float *keys,
                  const float *values, const float *q, const float *v, const float *conv_kernel, const float *conv_proj,
                  const float *align_prev, const float *align, const float *ctx, const float *dctx, const float *dalign_in,
                  float *dq, float *dkeys, float *dv_part, float *dconv_proj_part, float *dconv_kernel_part,
                  float *dalign_out, const float *znorm, void *ws, size_t ws_bytes, nabu_stream_t stream, unsigned *tickets,
                  float *ds_out = nullptr, float *cf_out = nullptr);
// slices of attn_param_grads' own frame partition; 0: that launch does not take the shape
int attn_defer_slices(const nabu_attn_desc *d);
int attn_param_grads(const nabu_attn_desc *d, int S, int L, const int32_t *dec_len, const int32_t *enc_len,
                     const float *keys, const float *q_all, const float *v, const float *wf, const float *ds_all,
                     const float *cf_all, float *dkeys, float *dv_part, float *dwf_part, hipStream_t s);

// out [C, R] = in [R, C]^T (row stride ldin)
int transpose(int R, int C, const float *in, int ldin, float *out, hipStream_t s);
// out[r][4u+g] = in[r][gU+u]: the gate-interleaved copy of a cell kernel's dense rows [R, 4U]
int permute_gates(int R, int U, const float *in, float *out, hipStream_t s);
// dst[r][c] += src[r][c] for row-strided [R, Cn] operands
int add_rows(int R, int Cn, const float *src, int lds, float *dst, int ldd, hipStream_t s);

}  // namespace nabu
