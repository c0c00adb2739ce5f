/* nabu_hip.h — C ABI of libnabu_hip.so: the MI355X (gfx950) kernels behind the
 * Nabu training hot path.
 *
 * The reference (vrenkens/nabu) has no FFI: its numerical backend is the
 * TensorFlow-1.8 op library, called from Python.  Each entry point below names
 * the reference call site (path relative to the reference root, file:line) whose
 * TF ops it replaces.  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *    the caller owns all memory, the library never allocates;
 *  - tensors are contiguous, batch-major, float32; lengths/labels are int32;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *  - return value: 0 = ok, < 0 = NABU_E* argument error, > 0 = hipError_t;
 *    nabu_last_error() returns a thread-local message;
 *  - no C++ exceptions cross the boundary;
 *  - state the library keeps between calls — all of it listed here: (process-wide, set
 *    before use, not synchronised) the default GEMM arithmetic (nabu_gemm_set_default_precision /
 *    NABU_GEMM_PRECISION) and the persistent kernels' wait bound (nabu_persist_set_timeout_us);
 *    (thread-local) the last error text, the profiling events of
 *    nabu_blstm_set_profile_events and the hook of nabu_blstm_set_phase_hook; plus a lazily built per-kernel attribute cache.  Everything
 *    else — parameters, activations, workspaces, status words — lives in caller-owned memory.
 */
#ifndef NABU_HIP_H
#define NABU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NABU_ABI_VERSION 4

#define NABU_EINVAL   (-1)  /* bad argument (shape, null pointer, alignment) */
#define NABU_EUNSUP   (-2)  /* shape not supported by the requested kernel   */
#define NABU_EWS      (-3)  /* workspace too small                           */

typedef void *nabu_stream_t; /* hipStream_t */

int nabu_version(void);
const char *nabu_last_error(void);

/* ------------------------------------------------------------------------
 * Dense fp32 GEMM on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32):
 *   C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] + beta * C + bias[N]
 * row-major; op(X) = X or X^T (trans* != 0 means the matrix is STORED
 * transposed, i.e. A is [K,M] / B is [N,K]).  bias may be NULL.
 * Segmented K (kseg > 0): the reduction index k runs over K = nseg*kseg rows
 * that are stored as nseg segments of kseg consecutive rows, segment s of A
 * starting a_seg_stride elements after segment s-1 (same for B); used for the
 * per-utterance shifted h_{t-1}^T·dz products.  Only valid with transA=1,
 * transB=0.  kseg = 0 means one contiguous segment.
 * Replaces: tf MatMul/BiasAdd inside LayerNormBasicLSTMCell._linear
 * (nabu/neuralnetworks/components/layer.py:35-47), tf.contrib.layers.linear
 * (models/ed_decoders/dnn_decoder.py:53-57), Dense layers of the attention
 * (components/attention.py:163-175) and their autodiff (trainers/trainer.py:556).
 * ws: split-K partial sums; query the size with nabu_gemm_ws_bytes. */
size_t nabu_gemm_ws_bytes(int M, int N, int K);
/* Arithmetic of the product (operands and result are fp32 in memory in every mode):
 *   NABU_GEMM_F32    exact fp32 on v_mfma_f32_32x32x2_f32 (the default);
 *   NABU_GEMM_BF16   operands rounded to bf16 inside the kernel, fp32 accumulation, on
 *                    v_mfma_f32_32x32x16_bf16 — the "bf16 MFMA input-to-hidden GEMMs" of
 *                    BASELINE.json configs[4];
 *   NABU_GEMM_BF16X3 / NABU_GEMM_BF16X6  each operand split into 2 / 3 bf16 pieces, 3 / 6 bf16
 *                    MFMA products: ~2^-16 / fp32-level (<= 2^-23) relative accuracy;
 *   NABU_GEMM_F16X3  fp32-level accuracy from three fp16 MFMA products of row-scaled two-plane operands
 *                    (nabu_pk_pack_f16 below): the BLSTM layer's time-batched products take it on packed
 *                    operands; a product on row-major operands (this function) computes bf16x6 instead.
 * NABU_GEMM_DEFAULT = the process default: NABU_GEMM_F32 unless changed by
 * nabu_gemm_set_default_precision() or the environment variable NABU_GEMM_PRECISION
 * (f32 | bf16 | bf16x3 | bf16x6 | f16x3).  Shapes the bf16 kernels do not take (K % 32, M % 4, N % 4,
 * unaligned operands) silently use the exact fp32 kernel — never a lower precision than asked. */
enum { NABU_GEMM_DEFAULT = 0, NABU_GEMM_F32 = 1, NABU_GEMM_BF16 = 2, NABU_GEMM_BF16X3 = 3, NABU_GEMM_BF16X6 = 4,
       NABU_GEMM_F16X3 = 5 };
int nabu_gemm_set_default_precision(int precision);
int nabu_gemm_get_default_precision(void);
int nabu_gemm_ex(int precision, int transA, int transB, int M, int N, int K, float alpha,
                 const float *A, int lda, const float *B, int ldb, float beta, float *C,
                 int ldc, const float *bias, int kseg, long long a_seg_stride,
                 long long b_seg_stride, void *ws, size_t ws_bytes, nabu_stream_t stream);
int nabu_gemm_f32(int transA, int transB, int M, int N, int K, float alpha,
                  const float *A, int lda, const float *B, int ldb, float beta,
                  float *C, int ldc, const float *bias, int kseg,
                  long long a_seg_stride, long long b_seg_stride, void *ws,
                  size_t ws_bytes, nabu_stream_t stream);

/* Decoder-step product: C[M,N] = [A | A2]·[B ; B2] + beta*C + bias for M <= 64 batch rows — the
 * reduction index runs over two operand pairs (the Speller cell's concat([context, h])·kernel,
 * nabu/neuralnetworks/models/ed_decoders/speller.py:33-45 -> tf LSTMCell's single matmul on the
 * concatenated input) without a concatenated copy, in ONE launch: workgroups own (column slice,
 * k-chunk) pairs, write their partial tiles through to memory, and the last arriver of a column
 * slice (a ticket per slice) sums the partials in chunk order — deterministic, no float atomics,
 * no separate reduce launch.  Requirements: N % 32 == 0, K1 and K2 multiples of 64 (K2 may be 0),
 * lda/lda2 % 4 == 0, 16-byte aligned operands; NABU_EUNSUP otherwise.  Exact fp32. */
size_t nabu_gemm2_ws_bytes(int M, int N, int K1, int K2);
int nabu_gemm2_f32(int M, int N, int K1, const float *A, int lda, const float *B, int ldb, int K2,
                   const float *A2, int lda2, const float *B2, int ldb2, float beta, float *C, int ldc,
                   const float *bias, void *ws, size_t ws_bytes, nabu_stream_t stream);

/* PACKED bf16-plane operands (gemm_pk.hip) — the time-batched input-to-hidden products and their
 * gradients on the bf16 matrix pipe at fp32-equivalent accuracy ("bf16x6", planes = 3) or in plain bf16
 * (planes = 1, BASELINE.json configs[4]).  An fp32 operand is converted ONCE per use-site into
 *     packed[kb][plane][row][16 k]   bf16; row = the operand's M (A) or N (B) index, padded to a multiple
 *                                    of 256 (nabu_pk_rows_pad); kb = k / 16, padded with zero blocks to
 *                                    nabu_pk_kblocks(K, planes); within a row's 32 bytes the two 16-byte
 *                                    halves are swapped when bit 3 of the row index is set;
 *     planes = 3: x = h + m + l with h = rne_bf16(x), m = rne_bf16(x - h), l = x - h - m (exact: the three
 *                 8-bit significands hold the 24 bits of x);  planes = 1: h only.
 * nabu_pk_pack writes one source matrix into a packed operand: rows [row_off, row_off + fill_rows) and
 * k-blocks [kb_off, kb_off + fill_kb), zeros where the source (R x C valid elements, row stride ld) ends.
 *   transposed = 0: packed row = source row, k = source column (fill_rows over R, fill_kb over ceil(C/16));
 *   transposed = 1: packed row = source column, k = source row (fill_rows over C, fill_kb over ceil(R/16));
 *                   with period > 0 the value at reduction index r is source row r + shift when
 *                   0 <= r % period + shift < period and 0 otherwise (the h_{t-1}^T·dz_t pairs of the
 *                   recurrent weight gradient: period = T, shift = -1 / +1 for the forward / backward cell).
 * nabu_gemm_pk: C_b[M,N] = alpha * sum_k A_b[m,k]·B_b[n,k] + beta*C_b + bias[n] for b < nbatch (<= 2), fp32
 * result; planes = 3 adds the six plane products h·h, h·m, m·h, m·m, h·l, l·h (v_mfma_f32_32x32x16_bf16, fp32
 * accumulation).  Columns n >= n_split (a multiple of 256, 0 = off) are written to C2_b[m, n - n_split] with
 * bias2 — one product fills the gate buffers of both directions.  Deterministic split-K through ws.
 * An operand packed with 3 planes can be used by a planes = 1 product (a_planes / b_planes = planes stored).
 * Replaces: the tf MatMul of LayerNormBasicLSTMCell._linear over all frames and its autodiff
 * (nabu/neuralnetworks/components/layer.py:35-47, nabu/neuralnetworks/trainers/trainer.py:556-558). */
typedef struct nabu_pk_gemm_desc {
  uint32_t size;          /* = sizeof(nabu_pk_gemm_desc) */
  int32_t planes;         /* 3 = bf16x6 (fp32-equivalent), 2 = f16x3 (fp32-equivalent, scaled fp16 planes), 1 = bf16 */
  int32_t M, N, nkb;      /* output size per batch entry; k-blocks of 16 to reduce over */
  int32_t nbatch;         /* 1 or 2 independent products in one launch */
  const void *A[2], *B[2];/* packed operands (first k-block of the reduction) */
  int32_t a_rows_pad, b_rows_pad, a_planes, b_planes;
  float *C[2], *C2[2];
  int32_t ldc, n_split;
  const float *bias, *bias2;
  float alpha, beta;
  const uint32_t *a_amax[2], *b_amax[2];  /* planes = 2: the row maxima the operands were packed with */
  int32_t direct;         /* planes = 2: 1 = chain the three plane products into the accumulators directly (three
                           * roundings of the matrix pipe per 16 k where the exact-fp32 instruction has eight; 10 %
                           * faster) instead of promoting 16-k partial sums (0, the default: one rounding per 16 k);
                           * 2 = direct when a workgroup's reduction is at most twice as long as the exact-fp32
                           * kernel's would be for the same product (fewer roundings than that kernel), else promoted */
} nabu_pk_gemm_desc;
int nabu_pk_rows_pad(int rows);
int nabu_pk_kblocks(int K, int planes);
size_t nabu_pk_bytes(int rows, int K, int planes);
int nabu_pk_pack(int planes, int transposed, const float *src, long long ld, int R, int C, void *dst,
                 int dst_rows_pad, int row_off, int kb_off, int fill_rows, int fill_kb, int period,
                 int shift, nabu_stream_t stream);
/* planes = 2, "f16x3": two scaled fp16 planes per operand and three plane products (l·h, h·l, h·h on
 * v_mfma_f32_32x32x16_f16) — half the matrix instructions of bf16x6 at the same error level.  Every packed ROW
 * (an M resp. N index, all its k) has a power-of-two scale 2^(14 - floor(log2 amax)) derived from `amax`, the
 * bit pattern of the row's largest magnitude: x·scale = h + l with h = rne_f16(x·scale), l = rne_f16(x·scale - h);
 * the product's epilogue divides the scales out.  amax[dst_rows_pad] (uint32, device) is indexed by packed row;
 * it comes from nabu_pk_amax (atomic maxima of the rows and / or columns of a source matrix into ZEROED arrays:
 * `rows[r]` for transposed = 0 packs, `cols[c]` for transposed = 1 packs) or from nabu_pk_amax_fill when a
 * bound is known a priori (LSTM outputs: 1).  Any upper bound of the row's magnitudes is valid; a bound 2^j too
 * large costs j bits of the l plane.  The same array goes into nabu_pk_gemm_desc.a_amax / b_amax. */
int nabu_pk_amax(const float *src, long long ld, int R, int C, uint32_t *rows, uint32_t *cols, nabu_stream_t stream);
int nabu_pk_amax_fill(uint32_t *dst, int n, float value, nabu_stream_t stream);
int nabu_pk_pack_f16(int transposed, const float *src, long long ld, int R, int C, void *dst, int dst_rows_pad,
                     int row_off, int kb_off, int fill_rows, int fill_kb, int period, int shift,
                     const uint32_t *amax, nabu_stream_t stream);
size_t nabu_gemm_pk_ws_bytes(const nabu_pk_gemm_desc *d);
int nabu_gemm_pk(const nabu_pk_gemm_desc *d, void *ws, size_t ws_bytes, nabu_stream_t stream);

/* out[n] = beta*out[n] + sum_m A[m*lda + n]  (bias gradients; deterministic
 * two-stage tree).  ws >= nabu_colsum_ws_bytes(M,N). */
size_t nabu_colsum_ws_bytes(int M, int N);
int nabu_colsum_f32(int M, int N, const float *A, int lda, float beta, float *out,
                    void *ws, size_t ws_bytes, nabu_stream_t stream);

/* A linear layer with a narrow output, y[M,N] = x[M,K]·W[K,N] + b with N <= 64 (the DNNDecoder's outlayer,
 * models/ed_decoders/dnn_decoder.py:53-57), exact fp32 (linear_narrow.hip).
 * Forward: nabu_gemm_ex / nabu_gemm_f32 take the narrow kernel by themselves when the arithmetic is fp32, N <= 64,
 * K % 4 == 0, lda % 4 == 0, A, B and C are 16-byte aligned, nothing is transposed, beta == 0 and kseg == 0: one launch,
 * no workspace, and a row's result does not depend on the rows it is computed with.
 * Backward: all three gradients from ONE pass over x and dy plus one small reduce launch,
 *   dx[M,K] = dy·W^T (dx may be NULL: skipped),  dW[K,N] = x^T·dy,  db[N] = colsum(dy),
 * dW (contiguous) and db OVERWRITTEN, as the beta = 0 calls they replace do.  Partial sums of dW and db go through ws
 * (nabu_linear_bwd_ws_bytes) and are added in a fixed order: bitwise repeatable, no float atomics.
 * NABU_EUNSUP: N > 64, K % 4 != 0, ldx or lddx % 4 != 0, an operand that is not 16-byte aligned, or NABU_LINEAR_NARROW=0
 * — the caller then makes the three calls (nabu_gemm_f32 twice, nabu_colsum_f32).
 * NABU_LINEAR_NARROW=0 (environment, read once) switches both kernels off: the products take the general tiles again. */
size_t nabu_linear_bwd_ws_bytes(int M, int K, int N);
int nabu_linear_bwd_f32(int M, int K, int N, const float *x, int ldx, const float *dy, int ldy,
                        const float *W, int ldw, float *dx, int lddx, float *dW, float *db, void *ws,
                        size_t ws_bytes, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * One bidirectional LSTM layer — layer.blstm
 * (nabu/neuralnetworks/components/layer.py:8-51): two
 * tf.contrib.rnn.LayerNormBasicLSTMCell(layer_norm=False) driven by
 * bidirectional_dynamic_rnn(sequence_length=len) and concatenated on the
 * feature axis.  Gate order i,j,f,o; forget bias +1 at run time; rows t >= len
 * produce 0 and freeze (c,h); the backward direction starts at each sequence's
 * own last frame.
 *   x [B,T,D], len [B], kernel_* [(D+H),4H], bias_* [4H], out [B,T,2H].
 * reserve (nabu_blstm_reserve_bytes) keeps the gate activations and cell states
 * for the backward pass; ws (nabu_blstm_ws_bytes) is scratch.
 * mode: NABU_LSTM_AUTO picks the persistent whole-sequence kernel when the
 * shape is supported, else one launch per timestep.
 * Persistent kernels, by shape (nabu_amd/csrc/), three families: H in {128, 256, 512} on a whole MI355X (256 CUs): the
 * recurrent product on the 16-bit matrix pipe as three fp16 plane products of row-scaled operands — lstm_persist_mxh.hip:
 * launches of up to 32 batch rows, 8 per unit, 16 hidden units per workgroup (a narrow first-layer input, D <= 64, is
 * projected inside the forward kernel); lstm_persist_mxf.hip: 33..64 rows at H = 512 as sixteen units of 8 rows, 32 hidden
 * units per workgroup; fp32-equivalent: outputs and gradients agree with the exact-fp32 kernels to rounding and are as
 * close to a float64 layer (tests/test_hip_fullsize.py, tests/test_hip_real_operands.py); larger batches as consecutive
 * launches; otherwise (H = 64, fewer CUs, NABU_PERSIST_MX=0, recurrent_precision = NABU_REC_F32) the exact-fp32
 * v_mfma_f32_4x4x1 kernels of lstm_persist.hip.  All need their whole grid co-resident: every launch is validated against
 * the occupancy query first (all chunks of a call before the first is enqueued) and NABU_LSTM_AUTO steps instead where it
 * does not fit. */
#define NABU_LSTM_AUTO       0
#define NABU_LSTM_STEPWISE   1
#define NABU_LSTM_PERSISTENT 2

/* nabu_blstm_desc.flags */
#define NABU_BLSTM_FWD_ONLY   1   /* no backward pass will follow (validation, decoding): the reserve holds the
                                     activations only — no room for the packed dZ^T / row maxima of the weight-gradient
                                     products (0.2-0.8 GB per cfg2 layer); nabu_blstm_bwd* reject such a descriptor */
/* nabu_blstm_desc.recurrent_precision */
#define NABU_REC_DEFAULT      0   /* the recurrent product h.W_h on the 16-bit matrix pipe: three fp16 plane products of
                                     row-scaled operands, fp32-equivalent (lstm_persist_mxh.hip / _mxf.hip) */
#define NABU_REC_F32          1   /* exact fp32 (v_mfma_f32_4x4x1, lstm_persist.hip): with gemm_precision = NABU_GEMM_F32
                                     the whole layer is float32 end to end, like layer.py:35-47 on TF's fp32 MatMul */

typedef struct {
  uint32_t size;      /* sizeof(nabu_blstm_desc), ABI versioning (the 32-byte layout of ABI version 1 — everything
                         up to gemm_precision — is still accepted: the fields behind it read as 0) */
  int32_t B, T, D, H;
  int32_t max_len;    /* max(len) if known on the host, else T */
  int32_t mode;       /* NABU_LSTM_* */
  int32_t gemm_precision; /* NABU_GEMM_* of the input-to-hidden products X·Wx, dZ·Wx^T, X^T·dZ
                             (BASELINE.json configs[4]: "bf16 MFMA input-to-hidden GEMMs");
                             the recurrent weight gradient H^T·dZ follows the process default */
  float x_bound;      /* > 0: the caller guarantees |x| <= x_bound for every element of the layer input — the previous
                         layer's LSTM outputs (|o tanh c| <= 1), after dropout 1 / keep_prob: the f16x3 packs of x take
                         their row scales from the bound and skip the measuring pass over x.  0: nothing is known, x is
                         measured (the first layer's features) */
  int32_t flags;      /* NABU_BLSTM_* */
  int32_t recurrent_precision;   /* NABU_REC_* */
  /* ---- ABI version 3 (the 44-byte layout of version 2 — everything up to recurrent_precision — is still accepted).
   * PACKED COMPANIONS of the layer's output and input.  With gemm_precision = NABU_GEMM_F16X3 every dense product of a
   * layer reads its operands as two fp16 planes (nabu_pk_pack_f16's layout); up to ABI version 2 each call converted
   * x, x^T and h^T itself, re-reading tensors the previous recurrent kernel had written microseconds earlier (0.44 ms of
   * a 12 ms cfg2 step).  |h| = |o tanh c| <= 1 is known a priori, so the forward recurrent kernel can write the planes
   * itself, next to `out`, at the scale 2^14 it already uses for its own exchange (row maxima = the bit pattern of
   * 1.0f for every packed row):
   *   out_pk_rows  `out` as the NEXT layer's input operand: rows = frames after stacking `out_stack` consecutive
   *                frames (ops.pyramid_stack, components/ops.py:6-60, as a view: T %% out_stack == 0), k = out_stack 2H;
   *                nabu_pk_bytes(B T / out_stack, out_stack 2H, 2) bytes
   *   out_pk_cols  the transposed operand of the same matrix (the next layer's x^T . dZ): nabu_pk_bytes(out_stack 2H,
   *                B T / out_stack, 2)
   *   hT_pk        this layer's own h_(t-1)^T operands of dWh, forward cell then backward cell, each
   *                nabu_pk_bytes(Mw, B T, 2), Mw = H (D + H where the first layer's x^T shares the operand: D < 256);
   *                written by nabu_blstm_fwd, read by nabu_blstm_bwd / _bwd_weights of the SAME descriptor
   *   x_pk_rows / x_pk_cols   this layer's input as the producer layer wrote it (its out_pk_rows / out_pk_cols): the
   *                call reads no fp32 x for its products
   * All optional (NULL = the call packs for itself, as before).  Buffers are caller-owned and must be ZERO-FILLED ONCE
   * before their first use (the kernels write only positions that exist: k-blocks beyond the reduction length and rows
   * beyond the operand stay zero) and may then be reused call after call.  nabu_blstm_fwd GUARANTEES the buffers it is
   * given are complete on return, whatever path it takes: written by the recurrent kernel where that is possible
   * (fp16-plane kernels, launches of <= 32 rows, max_len == T: nabu_blstm_emits_packed), by the pack kernels otherwise.
   * nabu_blstm_pk_bytes reports the sizes and whether the layer described would use the companions at all. */
  int32_t out_stack;            /* frames of `out` per packed row of out_pk_rows / out_pk_cols: 1 or 2 (0 reads as 1) */
  void *out_pk_rows;
  void *out_pk_cols;
  void *hT_pk;
  const void *x_pk_rows;
  const void *x_pk_cols;
} nabu_blstm_desc;

/* sizes of the packed companions of d (bytes; 0 where the layer described does not use that companion: another
 * gemm_precision, fewer than 2048 frames, an input of fewer than 256 features ...):
 *   bytes[0], bytes[1]  x_pk_rows, x_pk_cols as THIS layer would read them (its input [B, T, D])
 *   bytes[2]            hT_pk of this layer
 *   bytes[3], bytes[4]  out_pk_rows, out_pk_cols for d->out_stack (0 when T is not a multiple of it)
 * returns 0, or NABU_EINVAL for a bad descriptor */
int nabu_blstm_pk_bytes(const nabu_blstm_desc *d, size_t bytes[5]);
/* which of the companions d names nabu_blstm_fwd's recurrent kernel writes ITSELF: bit 0 out_pk_rows, bit 1 out_pk_cols,
 * bit 2 hT_pk (the others are made by pack kernels behind the recurrence — a caller that can pack lazily may prefer to
 * leave those out of the descriptor) */
int nabu_blstm_emits_packed(const nabu_blstm_desc *d);

/* RESERVE CONTRACT (since ABI version 2): nabu_blstm_fwd records, in host memory of THIS process, a fingerprint of the
 * layout it wrote (shape, planes, flags, recurrent_precision, sizes), keyed by the reserve's address; nabu_blstm_bwd /
 * _bwd_data / _bwd_weights compare it with the layout they derive and return NABU_EINVAL for a reserve that no forward
 * call of this process wrote, that was written under another layout (descriptor or process default precision changed
 * between the passes), or whose fingerprint has been displaced (the table keeps the 4096 most recently written
 * reserves).  A backward call therefore needs the forward call of the SAME process on the SAME address first; a
 * reserve copied elsewhere or produced by another process is rejected. */
size_t nabu_blstm_reserve_bytes(const nabu_blstm_desc *d);
size_t nabu_blstm_ws_bytes(const nabu_blstm_desc *d);
int nabu_blstm_fwd(const nabu_blstm_desc *d, const float *x, const int32_t *len,
                   const float *kernel_fw, const float *bias_fw,
                   const float *kernel_bw, const float *bias_bw, float *out,
                   void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream);
/* Gradient of nabu_blstm_fwd (autodiff of layer.blstm, trainers/trainer.py:556-558).
 * d_out [B,T,2H]; d_x [B,T,D] is overwritten (may be NULL for the first layer);
 * dkernel_*, dbias_* are overwritten.  reserve is consumed (overwritten). */
int nabu_blstm_bwd(const nabu_blstm_desc *d, const float *x, const int32_t *len,
                   const float *kernel_fw, const float *kernel_bw, const float *out,
                   const float *d_out, void *reserve, float *d_x, float *dkernel_fw,
                   float *dbias_fw, float *dkernel_bw, float *dbias_bw, void *ws,
                   size_t ws_bytes, nabu_stream_t stream);
/* The same gradient in two calls: nabu_blstm_bwd_data runs the recurrence backwards and produces what the layer
 * BELOW waits for (d_x) plus the bias gradients, leaving dz in `reserve`; nabu_blstm_bwd_weights turns that dz into
 * dkernel_fw / dkernel_bw ([(D+H),4H], overwritten) and may run any time later on the same stream with the same
 * x / out / reserve (a different ws is fine).  data + weights == nabu_blstm_bwd, bit for bit.  Why: nothing waits
 * for the weight gradients, and a long burst of bf16 matrix work in front of a latency-bound persistent recurrent
 * kernel slows that kernel down (the chip's clock recovers slowly: +0.5 ms on the 1000-frame layer of cfg2), so a
 * trainer runs the weight-gradient products of all layers after the last recurrence (TF's scheduler was free to
 * do the same with the MatMul gradients of trainers/trainer.py:556-558). */
int nabu_blstm_bwd_data(const nabu_blstm_desc *d, const float *x, const int32_t *len,
                        const float *kernel_fw, const float *kernel_bw, const float *out,
                        const float *d_out, void *reserve, float *d_x, float *dbias_fw, float *dbias_bw,
                        void *ws, size_t ws_bytes, nabu_stream_t stream);
int nabu_blstm_bwd_weights(const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *out,
                           void *reserve, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                           nabu_stream_t stream);

/* ---- layer-normalised BLSTM layer (lstm.hip's driver, lstm_ln.hip's recurrence): layer.blstm(layer_norm=True) ----
 * tf.contrib.rnn.LayerNormBasicLSTMCell(num_units, layer_norm=True) under bidirectional_dynamic_rnn.  Per direction,
 * batch row b and step s < len[b]:
 *   z = [x_t, h] . kernel                       (NO bias: the cell has no bias variable when it normalises)
 *   LN_k(v) = gamma_k (v - mean v) rsqrt(var v + 1e-12) + beta_k    over the H units of ONE gate (biased variance)
 *   c' = c sigmoid(LN_f(z_f) + 1) + sigmoid(LN_i(z_i)) tanh(LN_j(z_j));  c = LN_state(c')   (the normalised c is carried)
 *   h  = tanh(c) sigmoid(LN_o(z_o))
 * Steps s >= len[b]: output 0, state frozen; the backward direction runs over the reversed valid part (as nabu_blstm_fwd).
 * The norm parameters come in one struct: index 0..4 = input, transform, forget, output, state (the cell's scopes); every
 * array is [H].  The gradient pointers are read by the backward calls only and are overwritten.
 *
 * These entry points take nabu_blstm_desc as it is.  They are the exact-fp32, launch-per-step family: two launches per
 * step and pass (the recurrent product; the row statistics and the cell), both directions in each.  mode
 * NABU_LSTM_PERSISTENT is NABU_EUNSUP (the persistent kernels split H over workgroups and have no per-step
 * cross-workgroup reduction); AUTO and STEPWISE run the same kernels.  recurrent_precision is accepted and has no effect,
 * gemm_precision selects the arithmetic of x.Wx, dZ.Wx^T and x^T.dZ as in nabu_blstm_fwd (h^T.dZ is exact fp32), the
 * packed-companion fields are ignored (nothing is emitted or read packed).  H % 4 != 0 is NABU_EUNSUP.
 *
 * reserve = z_hat fw | bw [B,T,4H] (the normalised gate inputs; x.Wx before the recurrence, dZ - the gradient w.r.t. the
 * PRE-normalisation z - after the backward recurrence) | c_hat fw | bw [B,T,H] | rstd fw | bw [B,T,4] | rstd_c fw | bw
 * [B,T]; a NABU_BLSTM_FWD_ONLY descriptor's reserve is the gate buffers alone and nothing is saved.  The RESERVE CONTRACT
 * above holds here too (a table of its own: a reserve of nabu_blstm_fwd is rejected by these calls and vice versa).
 * The gamma/beta gradients are per-row running sums added up over the batch in a fixed order by one launch (no
 * floating-point atomics): two identical calls give identical bits. */
typedef struct nabu_blstm_ln_params {
  uint32_t size;             /* sizeof(nabu_blstm_ln_params) */
  uint32_t reserved;         /* 0 */
  const float *gamma[2][5];  /* [fw, bw][input, transform, forget, output, state], each [H] */
  const float *beta[2][5];
  float *dgamma[2][5];       /* backward: overwritten; forward: ignored (may be NULL) */
  float *dbeta[2][5];
} nabu_blstm_ln_params;
size_t nabu_blstm_ln_reserve_bytes(const nabu_blstm_desc *d);
size_t nabu_blstm_ln_ws_bytes(const nabu_blstm_desc *d);
int nabu_blstm_ln_fwd(const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *kernel_fw,
                      const float *kernel_bw, const nabu_blstm_ln_params *ln, float *out, void *reserve, void *ws,
                      size_t ws_bytes, nabu_stream_t stream);
/* d_x [B,T,D] is overwritten (may be NULL), dkernel_* [(D+H),4H] and the twenty dgamma / dbeta arrays are overwritten;
 * reserve is consumed.  _bwd_data (recurrence backwards, norm-parameter gradients, d_x; dZ stays in the reserve) followed
 * by _bwd_weights (dkernel_*; any time later on the same stream) == _bwd, bit for bit. */
int nabu_blstm_ln_bwd(const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *kernel_fw,
                      const float *kernel_bw, const nabu_blstm_ln_params *ln, const float *out, const float *d_out,
                      void *reserve, float *d_x, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                      nabu_stream_t stream);
int nabu_blstm_ln_bwd_data(const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *kernel_fw,
                           const float *kernel_bw, const nabu_blstm_ln_params *ln, const float *out, const float *d_out,
                           void *reserve, float *d_x, void *ws, size_t ws_bytes, nabu_stream_t stream);
int nabu_blstm_ln_bwd_weights(const nabu_blstm_desc *d, const float *x, const int32_t *len, const float *out,
                              void *reserve, float *dkernel_fw, float *dkernel_bw, void *ws, size_t ws_bytes,
                              nabu_stream_t stream);

/* 1 if nabu_blstm_fwd/bwd will run the persistent whole-sequence kernel for d. */
int nabu_blstm_uses_persistent(const nabu_blstm_desc *d);
/* Profiling hook (thread-local): when non-NULL, nabu_blstm_fwd/bwd record the
 * caller-owned hipEvent_t ev_begin right before and ev_end right after the
 * recurrent kernel(s) on the call's stream, so that bench.py can time the
 * dominant kernel live inside the timed region.  Pass NULLs to switch it off. */
int nabu_blstm_set_profile_events(void *ev_begin, void *ev_end);
/* Hook (thread-local) that nabu_blstm_bwd calls on the host right after it has enqueued the
 * recurrent kernel(s) and before it enqueues the dense products dWx, dWh, dx.  The persistent
 * recurrent kernels need every one of their workgroups resident at the same time, so nothing else
 * may run beside them; the products have no such constraint.  A data-parallel caller uses the hook
 * to start the all-reduce of an already finished gradient bucket on its communication stream at
 * exactly this point (ordered after the recurrence by an event) and joins that stream again before
 * the next recurrent launch — the exchange then overlaps the products only.  NULL switches it off.
 * Replaces: the asynchronous parameter-server pushes of the reference (trainers/trainer.py:479-510). */
typedef void (*nabu_phase_hook_t)(void *user);
int nabu_blstm_set_phase_hook(nabu_phase_hook_t fn, void *user);
/* Bound of every in-kernel wait of the persistent recurrent kernels (process-wide setting;
 * default 200 000 us, us <= 0 restores it).  A wait that runs out sets the status word (first
 * int32 of ws: 4*block + {1 forward, 2 backward, 3 start-up handshake}), every workgroup leaves at
 * its next barrier, later launches on that ws return at once until the caller has read and
 * cleared the word: the results of the step are invalid and the host must raise. */
int nabu_persist_set_timeout_us(long long us);

/* ops.pyramid_stack (nabu/neuralnetworks/components/ops.py:6-60) when T is not
 * a multiple of numsteps: y [B,Tp,F] = x [B,T,F] zero-padded in time (for T a
 * multiple the stack is a free view on the batch-major buffer).  The inverse
 * (gradient) drops the padded frames. */
int nabu_pad_time_f32(int B, int T, int Tp, int F, const float *x, float *y,
                      nabu_stream_t stream);
int nabu_unpad_time_f32(int B, int T, int Tp, int F, const float *y, float *x,
                        nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * CTC loss and gradient — loss_functions.CTC
 * (nabu/neuralnetworks/trainers/loss_functions.py:180-214): tf.nn.ctc_loss on
 * batch-major logits with blank = C-1, softmax inside, frames >= logit_len
 * ignored.  labels [B,Lmax] zero padded, label_len [B].
 *   nll [B]                     per-utterance -log p(labels | logits)
 *   dlogits [B,T,C]             grad_scale * d nll[b] / d logits  (0 past len)
 *   status [1] int32 (device)   set to 1+b if utterance b has no valid
 *                               alignment (TF raises in that case)
 * ws >= nabu_ctc_ws_bytes(B,T,Lmax). */
size_t nabu_ctc_ws_bytes(int B, int T, int Lmax);
int nabu_ctc_loss_grad(int B, int T, int C, int Lmax, const float *logits,
                       const int32_t *logit_len, const int32_t *labels,
                       const int32_t *label_len, float grad_scale, float *nll,
                       float *dlogits, int32_t *status, void *ws, size_t ws_bytes,
                       nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Forced alignment with a CTC model (ctc_align.hip): the best path through the lattice nabu_ctc_loss_grad sums over.
 * Same operands and conventions: raw batch-major logits [B,T,C], blank = C-1, labels [B,Lmax], frames >= logit_len
 * ignored.
 *
 * Definition.  ext[s] is the blank for even s and labels[s>>1] for odd s; S = 2L+1.  The recursion runs on the RAW
 * logits x, not on log-probabilities: every path visits every frame once, so the frame normalisers cannot change the
 * arg-max; leaving them out keeps exp and log out of the frame loop and makes ties well defined.
 *   v[0][0] = x[0][blank], v[0][1] = x[0][ext[1]], the rest unreachable;
 *   v[t][s] = x[t][ext[s]] + max over  stay s | step s-1 | skip s-2 (odd s with ext[s] != ext[s-2] only).
 * A tie keeps the SMALLER move: the step wins only if strictly greater than the stay, the skip only if strictly
 * greater than both.  The path ends in state S-1, unless S >= 2 and v[Tb-1][S-2] > v[Tb-1][S-1] strictly.
 * Unreachable is the finite -1e30 of nabu_ctc_loss_grad: it never wins against a reachable value, and no inf - inf
 * arises.
 *   state [B,T] int32     lattice state 0..2L of every frame, -1 from logit_len[b] on
 *   seg [B,Lmax,2] int32  first frame and last frame + 1 of label i; -1 beyond L
 *   conf [B,Lmax]         mean over the segment's frames of log softmax(x[t])[label] (0 beyond L)
 *   score [B]             sum over the frames of log softmax(x[t])[ext[state[t]]]
 * with log softmax evaluated as (x - mx) - lz, maximum and log-sum kept apart as in the loss.  score is summed in a
 * fixed order (a tree over frames) and conf in frame order, without floating-point atomics: identical calls give
 * identical bits.
 * An utterance with a label < 0 or >= C-1, logit_len <= 0, or label_len + adjacent repeats > logit_len (the loss's
 * test) gets score = -inf, state and seg -1, conf 0, and sets status [1] (device) to 1+b through
 * atomicCAS(status, 0, b+1), repeated while a later utterance holds the word: status names the FIRST such utterance
 * of the batch.  The other utterances are aligned normally.  L = 0 is valid: every frame is in state 0.
 * Routes: Lmax <= 63: one wave64 per utterance, two states per lane, no barrier in the frame loop; otherwise 256
 * threads with the states strided over them.  Back-pointers live in LDS while they fit and in ws otherwise;
 * NABU_CTC_ALIGN_WORKGROUP=1 forces the second route.  Every shape nabu_ctc_loss_grad's workgroup kernel takes is
 * taken.
 * NABU_EINVAL: a null pointer (labels may be null for Lmax = 0), B or T <= 0, C <= 1, Lmax < 0.  NABU_EWS:
 * ws_bytes < nabu_ctc_align_ws_bytes(B,T,Lmax) (0 for B or T <= 0 or Lmax < 0).  NABU_EUNSUP: more LDS than a
 * workgroup has, with the byte count in the message.  All three return before any launch. */
size_t nabu_ctc_align_ws_bytes(int B, int T, int Lmax);
int nabu_ctc_align(int B, int T, int C, int Lmax, const float *logits,
                   const int32_t *logit_len, const int32_t *labels,
                   const int32_t *label_len, int32_t *state, int32_t *seg, float *conf,
                   float *score, int32_t *status, void *ws, size_t ws_bytes,
                   nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * RNN transducer (Graves 2012, "Sequence Transduction with Recurrent Neural Networks") with the additive joint
 * (transducer.hip).  f [B,T,C] are the transcription logits, g [B,U1,C] the prediction logits (row u: the history
 * start symbol + labels[0..u)), blank = C-1, enc_len [B] the frames T_b (1..T), labels [B,ldl] (ldl >= U1-1; may be
 * null when U1 = 1), label_len [B] the labels U_b (0..U1-1).
 *
 * Definition.  h[t,u,k] = f[t,k] + g[u,k] (one float32 addition); log p(k|t,u) = (h[t,u,k] - mx[t,u]) - lz[t,u] with
 * mx the node's own maximum over k and lz = log sum_k exp(h - mx), kept apart as in the CTC loss; lb = log p(blank),
 * ly = log p(labels[u]).  h [B,T,U1,C] is never materialised.
 *   alpha[0,0] = 0,  alpha[t,u] = logadd(alpha[t-1,u] + lb[t-1,u], alpha[t,u-1] + ly[t,u-1])
 *   beta[T_b-1,U_b] = lb[T_b-1,U_b],  beta[t,u] = logadd(beta[t+1,u] + lb[t,u], beta[t,u+1] + ly[t,u])
 * Unreachable is the finite -1e30 of nabu_ctc_loss_grad.
 *   nll [B]        -beta[0,0] = -log sum over the monotone paths from (0,0) through the final blank at (T_b-1, U_b)
 *   df [B,T,C]     grad_scale * sum_u G[t,u,k]        dg [B,U1,C]   grad_scale * sum_t G[t,u,k]
 *   G[t,u,k] = exp(alpha[t,u] + beta[t,u] + nll) p(k|t,u) - [k = blank] exp(alpha[t,u] + lb[t,u] + beta[t+1,u] + nll)
 *                                                       - [k = labels[u]] exp(alpha[t,u] + ly[t,u] + beta[t,u+1] + nll)
 * with beta[T_b,U_b] read as 0 and every other beta outside the lattice as unreachable.  Rows of df from T_b on and
 * rows of dg past U_b are written as zeros: the caller need not clear anything.  Every sum runs in a fixed order
 * without floating-point atomics: identical calls give identical bits.
 * An utterance with a label < 0 or >= C-1, enc_len <= 0 or > T, or label_len < 0 or > U1-1 gets nll = 0 and zero
 * rows in df and dg, and sets status [1] (device) to 1+b through atomicCAS(status, 0, b+1), repeated while a later
 * utterance holds the word: status names the FIRST such utterance; the others are unaffected.  Any T_b >= 1 admits
 * every U_b: there is no "not enough frames" case.
 * Launches: emission terms (mx, lz, lb, ly of every node), the alpha and beta sweeps side by side, the gradients.
 * Routes of the sweeps: U1 <= 64: one wave64 per sweep and utterance walking anti-diagonals, lane u on node (d-u, u),
 * no barrier in the loop; otherwise 256 threads with u strided over them and a barrier per diagonal.  Both evaluate
 * the same per-node expression: same bits.  NABU_TRANSDUCER_WORKGROUP=1 (read once per process) forces the second.
 * NABU_TRANSDUCER_LAUNCHES (read on every call; for measurements only) is a mask of the launches to make: 1 emission
 * terms, 2 sweeps, 4 gradients; anything but 7 needs a workspace that a complete call on the same operands has filled.
 * NABU_EINVAL: a null pointer (labels may be null for U1 = 1), B, T or U1 <= 0, C <= 1, ldl < U1-1, B > 65535, or
 * T*U1 or B*(T+U1) >= 2^31.  NABU_EWS: ws_bytes < nabu_transducer_ws_bytes(B,T,U1) (0 for B, T or U1 <= 0).
 * NABU_EUNSUP: the second route with more than 150 KiB of LDS (8 U1 bytes).  All three return before any launch. */
size_t nabu_transducer_ws_bytes(int B, int T, int U1);
int nabu_transducer_loss_grad(int B, int T, int U1, int C, const float *f, const float *g,
                              const int32_t *enc_len, const int32_t *labels, int ldl,
                              const int32_t *label_len, float grad_scale, float *nll, float *df,
                              float *dg, int32_t *status, void *ws, size_t ws_bytes,
                              nabu_stream_t stream);
/* Forced alignment with a transducer model (transducer_align.hip): the best monotone path through the lattice
 * nabu_transducer_loss_grad sums over.  Same operands and conventions: f [B,T,C], g [B,U1,C], blank = C-1, enc_len
 * 1..T, labels [B,ldl] (may be null for U1 = 1), label_len 0..U1-1.
 *
 * Definition.  lb[t,u] and ly[t,u] are the loss's, made by the loss's own node expression: h = f + g is one float32
 * addition, log p = (h - mx) - lz with the node's own maximum and log-sum kept apart.  The frame normalisers depend on
 * (t,u), so the recursion runs on log-probabilities (nabu_ctc_align could use raw logits; this cannot):
 *   v[0,0] = 0,  v[t,u] = max(v[t-1,u] + lb[t-1,u], v[t,u-1] + ly[t,u-1])
 * with each candidate one float32 addition and unreachable the finite -1e30.  A tie keeps the BLANK move: the label
 * move wins only if strictly greater (nabu_ctc_align's "smaller move" rule).  A move that does not exist — the label
 * move in column 0, the blank move at frame 0 — is never taken whatever the back-pointer's comparison says, so with -inf or NaN terms (a
 * masked blank, a diverged model) the path still stays inside the lattice; its score, the sum of its terms, is then
 * -inf or NaN with status 0, as the loss returns nll = inf for such input.  The path ends with the blank at (T_b-1, U_b); the backtrace runs
 * from there to (0,0).
 *   state [B,T] int32     the u at which frame t's blank is taken = the labels emitted up to and including frame t;
 *                         -1 from enc_len[b] on; non-decreasing, state[T_b-1] = U_b
 *   frame [B,U1-1] int32  the frame at which label i is emitted = the first t with state[t] > i; -1 beyond U_b
 *   conf [B,U1-1]         ly[frame[i], i], the log-probability of label i at its emission node; 0 beyond U_b
 *   score [B]             the sum of the path's T_b + U_b terms: the log-probability of the best alignment
 * score is summed in a fixed order (a tree over the path's nodes) without floating-point atomics: identical calls give
 * identical bits.  frame and conf may be null for U1 = 1.
 * An utterance the loss rejects (a label < 0 or >= C-1, enc_len <= 0 or > T, label_len < 0 or > U1-1; the same test)
 * gets score = -inf, state and frame -1, conf 0, and sets status [1] (device) to 1+b through the loss's
 * atomicCAS rule: status names the FIRST such utterance; the others are aligned normally.  U_b = 0 is valid: every
 * state is 0.
 * Launches: emission terms (lb and ly only), then sweep, backtrace and outputs in one.  Routes of the sweep: U1 <= 64:
 * one wave64 per utterance walking anti-diagonals, lane u on node (d-u, u), the neighbour through DPP, no barrier in
 * the loop; otherwise 256 threads with u strided over them and a barrier per diagonal.  Both evaluate the same
 * per-node expression: same bits.  NABU_TRANSDUCER_ALIGN_WORKGROUP=1 (read once per process) forces the second.
 * Back-pointers (one bit per node) and the path live in LDS while they fit — nabu_transducer_align_lds_bytes(T, U1,
 * workgroup_route) <= 150 KiB — and in ws otherwise.  NABU_TRANSDUCER_ALIGN_LAUNCHES (read on every call; for
 * measurements only) is a mask of the launches to make: 1 emission terms, 2 sweep and backtrace; 2 alone needs a
 * workspace that a complete call on the same operands has filled.
 * NABU_EINVAL, NABU_EWS (ws_bytes < nabu_transducer_align_ws_bytes(B,T,U1), 0 for B, T or U1 <= 0) and NABU_EUNSUP
 * under nabu_transducer_loss_grad's conditions; all three return before any launch.  Every shape the loss takes is
 * taken. */
size_t nabu_transducer_align_ws_bytes(int B, int T, int U1);
size_t nabu_transducer_align_lds_bytes(int T, int U1, int workgroup_route);
int nabu_transducer_align(int B, int T, int U1, int C, const float *f, const float *g,
                          const int32_t *enc_len, const int32_t *labels, int ldl,
                          const int32_t *label_len, int32_t *state, int32_t *frame, float *conf,
                          float *score, int32_t *status, void *ws, size_t ws_bytes,
                          nabu_stream_t stream);
/* One step of the greedy transducer search for B rows in lock-step: one launch, one wave per row.  g_row [B,C] are
 * the prediction logits of each row's current history; t_pos, out_len [B], ids [B,S], last_id [B] and score [B] are
 * the search state, S the cap on labels per row.  step = 0 starts a search: the kernel itself sets t_pos = 0,
 * out_len = 0, score = 0, last_id = C-1 and ids = -1 before it decides, so the state needs no clearing; step > 0
 * continues from the state as found.
 * A row with t_pos >= enc_len or out_len >= S is finished: emit = 0 and nothing else is written.  Otherwise
 * k = argmax_k (f[b,t_pos,k] + g_row[b,k]) (one float32 addition; the smallest index among equal maxima),
 * score += (x_k - max) - log sum exp(x - max); k = blank: t_pos += 1, emit = 0; else ids[b,out_len++] = k,
 * last_id = k, emit = 1.  emit [B] can be passed as the seq_len of nabu_lstm_cell_fwd with step = 0: rows that
 * emitted advance the prediction network, the others copy their state through.
 * NABU_EINVAL before the launch: a null pointer, B, T or S <= 0, C <= 1, step < 0. */
int nabu_transducer_greedy_step(int B, int T, int C, int S, int step, const float *f,
                                const float *g_row, const int32_t *enc_len, int32_t *t_pos,
                                int32_t *out_len, int32_t *ids, int32_t *emit, int32_t *last_id,
                                float *score, nabu_stream_t stream);
/* One iteration of the alignment-length synchronous beam search of the transducer (Saon, Tueske and Audhkhasi 2020,
 * "Alignment-length synchronous decoding for RNN transducer"; transducer_beam.hip): one launch, one workgroup per
 * utterance.  At iteration i = step every active hypothesis with u labels sits at frame t = i - u (the frame is not
 * stored), so the whole beam of every utterance takes exactly one joint evaluation per iteration, and hypotheses that
 * spell the same labels meet at the same lattice node in the same iteration, where their probabilities are ADDED.
 *
 * Definition, per utterance b: el = min(max(enc_len[b], 0), T), blank = C-1, S the most labels a hypothesis may hold,
 * W the beam width.  step = 0 starts from the state as found, whatever it holds: the beam is the empty hypothesis in
 * slot 0 with score 0 and there are no finals; with el = 0 that hypothesis is complete at once: finals = [((), 0)] and
 * nothing is active.  Iteration i over the active hypotheses (y_w, s_w) in slots w = 0..n-1, each at t_w = i - |y_w| < el:
 *   1. log-probabilities: x = f[b,t_w,:] + g_rows[b,w,:] (one float32 addition), lp_w[k] = (x[k] - max x) - log sum exp(x - max x);
 *   2. candidates: v[w,k] = s_w + lp_w[k] for every class; a hypothesis with |y_w| = S has only its blank candidate;
 *   3. merge: for every pair of active hypotheses (a, c) with y_a = y_c + (k) — decided on the label sequences
 *      themselves — v[a,blank] = logadd(v[a,blank], v[c,k]) and candidate (c,k) is dropped;
 *      logadd(p, q) = max + log1p(exp(min - max)).  Active hypotheses are pairwise distinct: an a has one partner at most;
 *   4. order: the remaining candidates by value, largest first, equal values by flat index w C + k, smallest first; the
 *      first W are taken, or fewer if fewer exist;
 *   5. placement, in that order: a blank candidate with t_w + 1 = el COMPLETES y_w: it is offered to the finals and takes
 *      no active slot (the beam shrinks); any other blank gives the active (y_w, v) with parent = w, emit = 0,
 *      last_id = blank; a label gives (y_w + k, v) with parent = w, emit = 1, last_id = k.  New actives fill slots
 *      0, 1, .. in selection order; every other slot is empty: out_len = -1, ids = -1, score = -inf, parent = its own
 *      index, emit = 0, last_id = blank;
 *   6. finals: at most W are kept, best score first, in slots 0, 1, ..; a completed hypothesis goes in behind finals of
 *      equal score, what falls past W is dropped; empty slots have fin_len = -1, fin_ids = -1, fin_score = -inf.
 * An utterance is done when it has no active hypothesis, after at most el + S iterations (one still active at iteration
 * el + S would need t >= el); at least one final exists by then.  The result is the best final, fin_*[b,0].
 * Consequences (each checked with the float64 restatement, tests/transducer_beam_ref.py):
 *   - unpruned search gives exact scores: with W at least the number of label sequences of length <= S the final score
 *     of every y is log P(y | x), what nabu_transducer_loss_grad returns as -nll;
 *   - W = 1 takes the decisions of nabu_transducer_greedy_step (the same tie rule: the blank has the largest index):
 *     labels and lengths are equal, and the score wherever the row ran out of frames.  A row that the greedy search
 *     stops at S labels with frames left goes on through blanks here, which the greedy search never pays for;
 *   - merging matters: it changes which hypothesis is best, not only the scores.
 * ids [B,W,S] (padded with -1), out_len, score [B,W] are the beam, updated in place; the survivors' label rows are made
 * from the parents' rows as found (staged in LDS), so a parent may feed several children and slots may permute.  parent,
 * emit, last_id [B,W] are what the prediction network needs next: gather its state rows by parent, then advance the
 * rows with emit = 1 on last_id (emit can be the seq_len of nabu_lstm_cell_fwd at step 0).  g_rows [B,W,C] holds the
 * prediction logits of the hypothesis in each slot.  f and g_rows of empty slots are never read, nor is f beyond el.
 * A slot whose out_len is outside 0..S or whose frame step - out_len is outside 0..el-1 counts as empty.
 * The log-sum-exp of a hypothesis is taken by one wave, lane-strided over C; the selection is W rounds of a block-wide
 * arg-max over the candidates in LDS; no sum is atomic: two calls give the same bits.
 * ws: the finals' label rows while they are reordered, nabu_transducer_beam_ws_bytes(B,W,C,S) bytes (0 for a dimension <= 0).
 * NABU_EINVAL: W outside 1..32, B outside 1..65535, T < 1, S < 1, C < 2, step < 0, a null pointer.  NABU_EWS: ws_bytes too
 * small.  NABU_EUNSUP: 4 W (C + S) bytes of LDS are more than a CU has.  All three return before any launch. */
size_t nabu_transducer_beam_ws_bytes(int B, int W, int C, int S);
int nabu_transducer_beam_step(int B, int T, int C, int S, int W, int step, const float *f,
                              const float *g_rows, const int32_t *enc_len, int32_t *ids,
                              int32_t *out_len, float *score, int32_t *parent, int32_t *emit,
                              int32_t *last_id, int32_t *fin_ids, int32_t *fin_len, float *fin_score,
                              void *ws, size_t ws_bytes, nabu_stream_t stream);

/* Masked sparse softmax cross-entropy averaged over the target length —
 * loss_functions.average_cross_entropy / cross_entropy
 * (nabu/neuralnetworks/trainers/loss_functions.py:78-109,155-165):
 *   loss[b]    = sum_{t<logit_len[b]} xent(logits[b,t], targets[b,t]) / target_len[b]
 *   dlogits    = grad_scale * d loss[b] / d logits   (0 for t >= logit_len[b])
 * logits [B,L,C]; targets [B,ldt] int32 with ldt >= L. */
int nabu_xent_loss_grad(int B, int L, int C, int ldt, const float *logits,
                        const int32_t *targets, const int32_t *logit_len,
                        const int32_t *target_len, float grad_scale, float *loss,
                        float *dlogits, nabu_stream_t stream);

/* The same loss against label-smoothed targets (the [trainer] key label_smoothing; the rule of
 * tf.losses.softmax_cross_entropy(label_smoothing=...)): with C classes the target of a frame with label y is
 *   q = (1 - smoothing) * onehot(y) + smoothing / C          (the mass is spread over all C classes, y included)
 * and per frame t inside the mask, lz = logsumexp(x), xm = mean_c x_c, s = grad_scale / target_len[b]:
 *   loss_t = lz - (1 - smoothing) * x_y - smoothing * xm
 *   d_c    = s * (softmax_c - (1 - smoothing) * [c = y] - smoothing / C)
 * Mask, divisor and the zero rows past the mask are nabu_xent_loss_grad's; the row sum rides in the kernel's sum-exp
 * loop.  0 <= smoothing < 1, NABU_EINVAL otherwise (and for NaN); smoothing = 0 launches nabu_xent_loss_grad's own
 * instantiation: bit-identical loss and dlogits. */
int nabu_xent_smooth_loss_grad(int B, int L, int C, int ldt, const float *logits,
                               const int32_t *targets, const int32_t *logit_len,
                               const int32_t *target_len, float grad_scale, float smoothing,
                               float *loss, float *dlogits, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Speller decoder step kernels — RNNDecoder._decode / Speller.create_cell
 * (nabu/neuralnetworks/models/ed_decoders/rnn_decoder.py:13-82, speller.py:13-69):
 * tf.contrib.rnn.LSTMCell inside tf.contrib.seq2seq.AttentionWrapper driven by
 * dynamic_decode(impute_finished=True).  The dense products of a step run on
 * nabu_gemm_f32; these are the fused non-GEMM parts.
 *
 * nabu_lstm_cell_fwd: z [B,4U] = (dense part of) [inputs, h]·kernel; adds bias [4U]
 *   and, when emb_rows != NULL, row ids[b] of emb_rows [C,4U] (the one-hot input
 *   times the kernel is a row gather); gate order i,j,f,o, forget bias +1;
 *   acts [B,4U] keeps (i,g,f,o) for the gradient; rows with step >= seq_len[b] are
 *   finished: state copied through, acts = 0.
 * nabu_lstm_cell_bwd: dz [B,4U] from dh (+ dh2 if not NULL), dc_in and the saved
 *   acts / cell states; dc_out is the cell gradient handed to step-1. */
int nabu_lstm_cell_fwd(int B, int U, int step, const int32_t *seq_len, const float *z,
                       const float *bias, const float *emb_rows, const int32_t *ids,
                       const float *c_prev, const float *h_prev, float *acts,
                       float *c_new, float *h_new, nabu_stream_t stream);
int nabu_lstm_cell_bwd(int B, int U, int step, const int32_t *seq_len, const float *acts,
                       const float *c_new, const float *c_prev, const float *dh,
                       const float *dh2, const float *dc_in, float *dz, float *dc_out,
                       nabu_stream_t stream);

/* Fused attention step — attention.factory 'vanilla' (tf BahdanauAttention) and
 * 'location_aware' (nabu/neuralnetworks/components/attention.py:6-39,90-240):
 *   score[b,t] = sum_u v[u] * tanh(keys[b,t,u] + q[b,u] (+ f[b,t,u]))
 *   f = conv1d(align_prev, conv_kernel [K,F], 'same') · conv_proj [F,U]   (location)
 *   align = softmax over t < enc_len[b] (score mask -inf), ctx = align^T · values
 * keys [B,Te,U] (= values·memory_kernel, one GEMM per batch), values [B,Te,E]
 * (rows >= enc_len are zero), q [B,U] (= h·query_kernel).  Rows with
 * step >= dec_len[b] are finished: align/ctx copy align_prev/ctx_prev.
 * The backward kernel recomputes tanh, ACCUMULATES into dkeys [B,Te,U] and into the
 * partials dv_part [B*S,U], dconv_proj_part [B*S,F,U], dconv_kernel_part
 * [B,K,F] (the caller zeroes them before the first step and column-sums them
 * afterwards; S below), writes dq [B,U] and dalign_out [B,Te] (gradient w.r.t. align_prev;
 * location only).  dalign_in (may be NULL) is the gradient that reaches this
 * step's alignments through the next step's location features.
 * probability_fn: alignments = softmax(score) | sigmoid(score) | sigmoid(score) / sum_t sigmoid(score)
 * over the unmasked frames (masked frames get 0).  normalized_sigmoid keeps its normaliser per
 * utterance in znorm [B] (written by the forward kernel, read by the backward kernel; NULL otherwise).
 * 'windowed' (WindowedAttention, attention.py:294-396) is the vanilla score restricted to the
 * frames [m - left - 1, m + right), m = the first frame at which the cumulated PREVIOUS alignment
 * exceeds 0.5 (Te if none does); the initial alignment is one-hot at frame 0 (the decoder drivers
 * set it).  The window is a constant of the step: the backward kernel is the vanilla one. */
typedef struct {
  uint32_t size;       /* sizeof(nabu_attn_desc) */
  int32_t B, Te, E, U;
  int32_t kind;        /* 0 = vanilla (Bahdanau), 1 = location_aware, 2 = windowed */
  int32_t K, F;        /* location_aware: filtersize, numfilt; windowed: left_window_width, right_window_width */
  int32_t prob_fn;     /* probability_fn (attention.py:9-13): 0 softmax, 1 sigmoid, 2 normalized_sigmoid */
} nabu_attn_desc;
int nabu_attn_fwd(const nabu_attn_desc *d, int step, const int32_t *dec_len,
                  const int32_t *enc_len, const float *keys, const float *values,
                  const float *q, const float *v, const float *conv_kernel,
                  const float *conv_proj, const float *align_prev, const float *ctx_prev,
                  float *align, float *ctx, float *znorm, void *ws, size_t ws_bytes,
                  nabu_stream_t stream);
/* bytes of ws the forward pass needs (0 when the batch alone fills the chip): small batches are cut
 * into slices of encoder frames like the backward pass, partial softmax sums / contexts meet in ws */
size_t nabu_attn_fwd_ws_bytes(const nabu_attn_desc *d);
/* The backward pass cuts every utterance into S = nabu_attn_bwd_slices(d) slices of encoder frames
 * (one workgroup each, so that a step fills the chip at small batch sizes): dv_part and
 * dconv_proj_part have B*S rows; ctx is THIS step's context (the forward output: it turns the
 * softmax's sum over all frames into a dot product, which is what makes the slices independent);
 * ws (nabu_attn_bwd_ws_bytes) holds the per-slice dq and the d location features. */
int nabu_attn_bwd_slices(const nabu_attn_desc *d);
size_t nabu_attn_bwd_ws_bytes(const nabu_attn_desc *d);
int nabu_attn_bwd(const nabu_attn_desc *d, int step, const int32_t *dec_len,
                  const int32_t *enc_len, const float *keys, const float *values,
                  const float *q, const float *v, const float *conv_kernel,
                  const float *conv_proj, const float *align_prev, const float *align,
                  const float *ctx, const float *dctx, const float *dalign_in, float *dq,
                  float *dkeys, float *dv_part, float *dconv_proj_part,
                  float *dconv_kernel_part, float *dalign_out, const float *znorm, void *ws,
                  size_t ws_bytes, nabu_stream_t stream);

/* Whole-sequence decoder driver: RNNDecoder._decode over all L = max(dec_len)
 * steps in one call (rnn_decoder.py:59-82: ScheduledEmbeddingTrainingHelper,
 * BasicDecoder, dynamic_decode(impute_finished=True)),
 * i.e. per step: recurrent GEMMs + nabu_lstm_cell_fwd per layer (optional output
 * dropout, speller.py:38-43), query GEMM, nabu_attn_fwd (with sample_prob > 0 also the step's
 * projection + nabu_sample_ids for the next input); then ONE projection GEMM for
 * all steps (rnn_cell.py:145-155).  nabu_speller_bwd is its gradient; weight
 * gradients that are sums over steps are single GEMMs over all steps.
 *   values [B,Te,E] encoder output (rows >= enc_len zero), ids [L,B] decoder input
 *   labels (row 0 = C-1, then the targets shifted by one), logits [B,L,C].
 * With one layer, softmax attention (vanilla; forward also location-aware), no dropout / sampling and B = 32 (forward:
 * or 64) the L steps of the forward and of the backward pass are ONE persistent launch each (speller_persist.hip; NABU_SPELLER_PERSIST=0 /
 * NABU_SPELLER_PERSIST_BWD=0 keep the per-step kernels).
 * Its in-kernel waits are bounded like those of the recurrent layers: ws[0] (int32) is its status word,
 * 0 = ok, sticky — provide the workspace zero-initialised once; a non-zero word means a launch gave up
 * (results invalid) and makes later launches on that workspace return at once.
 * Kernel layouts are TF's: lstm_kernel[0] [(C+E+U),4U] (rows: one-hot, context, h),
 * lstm_kernel[n>0] [(2U),4U], memory_kernel [E,U], query_kernel [U,U], attention_v [U],
 * conv_kernel [K,F], conv_proj [F,U], out_kernel [(U+E),C] (rows: h, context), out_bias [C]. */
#define NABU_SPELLER_MAX_LAYERS 4
typedef struct {
  uint32_t size;
  int32_t B, Te, E, U, C, L, num_layers;
  int32_t kind, K, F, prob_fn;        /* attention: see nabu_attn_desc */
  float keep_prob;                    /* output dropout of every LSTM layer; 1 = off */
  unsigned long long seed, seed_offset;
  float sample_prob;                  /* scheduled sampling probability (speller.cfg sample_prob); 0 = off */
  unsigned long long sample_seed, sample_offset;
} nabu_speller_desc;
typedef struct {
  const float *memory_kernel, *query_kernel, *attention_v, *conv_kernel, *conv_proj, *out_kernel, *out_bias;
  const float *lstm_kernel[NABU_SPELLER_MAX_LAYERS], *lstm_bias[NABU_SPELLER_MAX_LAYERS];
} nabu_speller_params;
typedef struct {
  float *memory_kernel, *query_kernel, *attention_v, *conv_kernel, *conv_proj, *out_kernel, *out_bias;
  float *lstm_kernel[NABU_SPELLER_MAX_LAYERS], *lstm_bias[NABU_SPELLER_MAX_LAYERS];
} nabu_speller_grads;
/* Scheduled sampling — tf.contrib.seq2seq.ScheduledEmbeddingTrainingHelper as used by
 * rnn_decoder.py:59-66: after step t, row b draws select ~ Bernoulli(sample_prob); if selected
 * the decoder input of step t+1 is a sample from Categorical(softmax(logits_t[b])) instead of
 * the target y_t (no gradient flows through the sample).
 *   out_ids[b] = select ? sample : teacher_ids[b];  logits [B,C];
 * Philox4x32-10, counter (b, offset), key seed: a pure function of its arguments. */
int nabu_sample_ids(int B, int C, const float *logits, float prob, unsigned long long seed,
                    unsigned long long offset, const int32_t *teacher_ids, int32_t *out_ids,
                    nabu_stream_t stream);
/* The decoder inputs actually used by the last nabu_speller_fwd on `reserve` ([L,B] int32,
 * equal to `ids` when sample_prob == 0), copied to out_ids (device). */
int nabu_speller_decoder_inputs(const nabu_speller_desc *d, const void *reserve, int32_t *out_ids,
                                nabu_stream_t stream);
size_t nabu_speller_reserve_bytes(const nabu_speller_desc *d);
size_t nabu_speller_ws_bytes(const nabu_speller_desc *d);
/* 1 when the decoder steps of this descriptor run as ONE persistent launch (speller_persist.hip) in the forward
 * (backward = 0) resp. backward pass on the current device, 0 when they take the step chain.  Diagnostic: the two
 * paths compute the same function (tests/test_hip_speller.py compares them). */
int nabu_speller_uses_persistent(const nabu_speller_desc *d, int backward);
int nabu_speller_fwd(const nabu_speller_desc *d, const float *values, const int32_t *enc_len,
                     const int32_t *ids, const int32_t *dec_len, const nabu_speller_params *p,
                     float *logits, void *reserve, void *ws, size_t ws_bytes, nabu_stream_t stream);
/* every gradient buffer is overwritten; dvalues [B,Te,E] */
int nabu_speller_bwd(const nabu_speller_desc *d, const float *values, const int32_t *enc_len,
                     const int32_t *ids, const int32_t *dec_len, const nabu_speller_params *p,
                     const float *dlogits, void *reserve, const nabu_speller_grads *g,
                     float *dvalues, void *ws, size_t ws_bytes, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Speller over M encoded inputs, one attention mechanism each — Speller.create_cell with several
 * entries in `encoded` (nabu/neuralnetworks/models/ed_decoders/speller.py:49-61: one attention.factory
 * per encoded input, the list handed to tf.contrib.seq2seq.AttentionWrapper, AttentionProjectionWrapper
 * on [cell_output, contexts]).  Memory m has its own Te[m], E[m], enc_len and variables; the attention
 * type, probability_fn, K / F and num_units are shared (every mechanism is built from one [decoder] conf).
 * Per step: cell input [onehot | ctx_0 | .. | ctx_{M-1}], q_m = h_top . query_kernel[m], align_m / ctx_m
 * exactly as nabu_attn_fwd defines them, logits = [h_top | ctx_0 | .. | ctx_{M-1}] . out_kernel + out_bias.
 *   lstm_kernel[0] [(C + sum E + U), 4U] (rows: one-hot, contexts in mechanism order, h),
 *   out_kernel [(U + sum E), C] (rows: h, contexts in mechanism order); the rest per mechanism as nabu_speller_params.
 *   values / enc_len / dvalues: HOST arrays of M device pointers ([B,Te[m],E[m]] / [B]).
 * M <= NABU_SPELLER_MAX_MEMORIES = 4 (a launch's mechanism table travels as a kernel argument).
 * The decoder steps always run as the step chain (nabu_speller_multi_uses_persistent == 0: neither the
 * persistent decoder nor the matrix-pipe location-aware kernels are extended to several memories).  A step's M
 * attention mechanisms are ONE launch per pass (a grid dimension selects the mechanism; a workgroup reads
 * its memory's Te, E and pointers from the table), the contexts live in one [B, sum E] buffer that is the
 * operand of the next step's cell product and of the projection, and the M queries are one product against
 * the column-concatenated [U, M U] query kernels.  No floating-point atomics: identical calls, identical bits.
 * reserve_bytes == 0 together with nabu_last_error() is the "unsupported shape" answer. */
#define NABU_SPELLER_MAX_MEMORIES 4
typedef struct {
  uint32_t size;
  int32_t M;                                   /* number of encoded inputs, 1..NABU_SPELLER_MAX_MEMORIES */
  int32_t B, U, C, L, num_layers;
  int32_t Te[NABU_SPELLER_MAX_MEMORIES], E[NABU_SPELLER_MAX_MEMORIES];
  int32_t kind, K, F, prob_fn;                 /* attention: see nabu_attn_desc */
  float keep_prob;
  unsigned long long seed, seed_offset;
  float sample_prob;
  unsigned long long sample_seed, sample_offset;
} nabu_speller_multi_desc;
typedef struct {
  const float *memory_kernel[NABU_SPELLER_MAX_MEMORIES], *query_kernel[NABU_SPELLER_MAX_MEMORIES],
      *attention_v[NABU_SPELLER_MAX_MEMORIES], *conv_kernel[NABU_SPELLER_MAX_MEMORIES],
      *conv_proj[NABU_SPELLER_MAX_MEMORIES];
  const float *out_kernel, *out_bias;
  const float *lstm_kernel[NABU_SPELLER_MAX_LAYERS], *lstm_bias[NABU_SPELLER_MAX_LAYERS];
} nabu_speller_multi_params;
typedef struct {
  float *memory_kernel[NABU_SPELLER_MAX_MEMORIES], *query_kernel[NABU_SPELLER_MAX_MEMORIES],
      *attention_v[NABU_SPELLER_MAX_MEMORIES], *conv_kernel[NABU_SPELLER_MAX_MEMORIES],
      *conv_proj[NABU_SPELLER_MAX_MEMORIES];
  float *out_kernel, *out_bias;
  float *lstm_kernel[NABU_SPELLER_MAX_LAYERS], *lstm_bias[NABU_SPELLER_MAX_LAYERS];
} nabu_speller_multi_grads;
size_t nabu_speller_multi_reserve_bytes(const nabu_speller_multi_desc *d);
size_t nabu_speller_multi_ws_bytes(const nabu_speller_multi_desc *d);
/* always 0 (see above); the query exists so that a caller can ask both decoders the same question */
int nabu_speller_multi_uses_persistent(const nabu_speller_multi_desc *d, int backward);
/* frame slices per utterance of mechanism m's attention workgroups (1: the batch alone fills the chip) */
int nabu_speller_multi_attn_slices(const nabu_speller_multi_desc *d, int m);
int nabu_speller_multi_fwd(const nabu_speller_multi_desc *d, const float *const *values_host,
                           const int32_t *const *enc_len_host, const int32_t *ids, const int32_t *dec_len,
                           const nabu_speller_multi_params *p, float *logits, void *reserve, void *ws,
                           size_t ws_bytes, nabu_stream_t stream);
/* every gradient buffer is overwritten; dvalues_host[m] -> [B,Te[m],E[m]] */
int nabu_speller_multi_bwd(const nabu_speller_multi_desc *d, const float *const *values_host,
                           const int32_t *const *enc_len_host, const int32_t *ids, const int32_t *dec_len,
                           const nabu_speller_multi_params *p, const float *dlogits, void *reserve,
                           const nabu_speller_multi_grads *g, float *const *dvalues_host, void *ws,
                           size_t ws_bytes, nabu_stream_t stream);
/* Beam search over M encoded inputs: the loop of nabu_speller_beam_search (one function for both entry points: same
 * pruning, stop test and outputs) with the cell above on B*beam_width rows and the step's M attention mechanisms as
 * one launch, also for M = 1; the M alignment states are pruned and gathered per memory and
 * alignments_host[m] (may be NULL as a whole) receives [B,W,max_steps,Te[m]]. */
typedef struct {
  uint32_t size;
  int32_t M, B, U, C, num_layers;
  int32_t Te[NABU_SPELLER_MAX_MEMORIES], E[NABU_SPELLER_MAX_MEMORIES];
  int32_t kind, K, F, prob_fn, beam_width, max_steps;
  float length_penalty, temperature;
} nabu_multi_beam_desc;
size_t nabu_speller_multi_beam_ws_bytes(const nabu_multi_beam_desc *d);
int nabu_speller_multi_beam_search(const nabu_multi_beam_desc *d, const float *const *values_host,
                                   const int32_t *const *enc_len_host, const nabu_speller_multi_params *p,
                                   int32_t *sequences, int32_t *lengths, float *scores,
                                   float *const *alignments_host, int32_t *num_steps, void *ws, size_t ws_bytes,
                                   nabu_stream_t stream);
/* Sampled decoding over M encoded inputs: nabu_speller_sample (below) with the cell and the attention launch of the
 * search above, also for M = 1; alignments_host[m] (may be NULL as a whole) receives [B,max_steps,Te[m]]. */
size_t nabu_speller_multi_sample_ws_bytes(const nabu_multi_beam_desc *d);
int nabu_speller_multi_sample(const nabu_multi_beam_desc *d, const float *const *values_host,
                              const int32_t *const *enc_len_host, const nabu_speller_multi_params *p,
                              unsigned long long seed, unsigned long long offset0, int32_t *sequences,
                              int32_t *lengths, float *nll, float *const *alignments_host, int32_t *num_steps,
                              void *ws, size_t ws_bytes, nabu_stream_t stream);
int nabu_speller_multi_decoder_inputs(const nabu_speller_multi_desc *d, const void *reserve, int32_t *out_ids,
                                      nabu_stream_t stream);

/* x[b,t,:] = 0 for t >= len[b] (dynamic_decode zeroes the outputs of finished rows). */
int nabu_mask_time_f32(int B, int L, int F, float *x, const int32_t *len, nabu_stream_t stream);
/* y[b,l,:] = x[l,b,:] (time-major per-step buffers <-> the batch-major API). */
int nabu_swap01_f32(int L, int B, int F, const float *x, float *y, nabu_stream_t stream);
/* dK[c,:] = sum_{i: ids[i]==c} dz[i,:]  (gradient of the kernel rows gathered by the
 * one-hot decoder inputs), ids [N], dz [N,W], dK [C,W]; deterministic. */
int nabu_scatter_rows_f32(int C, int N, int W, const int32_t *ids, const float *dz, float *dK,
                          nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused per-element gradient clip + TF-style Adam on flat buffers —
 * Trainer._update (nabu/neuralnetworks/trainers/trainer.py:525,560-569):
 *   g = clamp(grad_scale*grad, -clip, clip); m = b1 m + (1-b1) g;
 *   v = b2 v + (1-b2) g^2; param -= lr_t * m / (sqrt(v) + eps)
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller. */
int nabu_adam_clip_step(size_t n, float *param, const float *grad, float *m,
                        float *v, float lr_t, float b1, float b2, float eps,
                        float clip, float grad_scale, nabu_stream_t stream);
/* The same update with the parameter read from a separate, read-only source:
 *   param_out = src - lr_t * m / (sqrt(v) + eps)
 * (m, v updated in place as above; src and param_out must not overlap).  The optimiser of a weight-noise step
 * (nabu_weight_noise_f32 below): the gradient was taken at param_out = src + noise, the update starts from the clean
 * src — no restoring pass and no (w + n) - n arithmetic, which is not exact in float32.  With src a copy of param the
 * results equal nabu_adam_clip_step's bit for bit. */
int nabu_adam_clip_step_from(size_t n, float *param_out, const float *src, const float *grad, float *m,
                             float *v, float lr_t, float b1, float b2, float eps,
                             float clip, float grad_scale, nabu_stream_t stream);
/* g = clamp(g, -clip, clip) in place (data-parallel mode clips per replica
 * BEFORE the all-reduce, trainer.py:556-569). */
int nabu_clip_f32(size_t n, float *g, float clip, nabu_stream_t stream);

/* Gradient accumulation (numbatches_to_aggregate = A * replicas, A > 1: Trainer.step_accumulated).  Every backward
 * pass OVERWRITES the flat gradient buffer (the weight-gradient products run with beta = 0, the bias and norm-parameter
 * gradients are plain column sums, nothing is added to what the buffer held), so the sum over an update's micro-batches
 * is kept in a second flat buffer.  Each micro-batch's gradient is clipped as a replica's is before the exchange and
 * added in the fixed order j = 0, 1, ...:
 *   out[i] = clamp(g[i], -clip, clip) + (acc ? acc[i] : 0)
 * acc = NULL is the first micro-batch: a pure write, the accumulator is neither cleared nor read.  out may be acc (the
 * usual case) or g (the last micro-batch of a data-parallel update, whose local sum is exchanged from the gradient
 * buffer) or a buffer of its own; a shifted overlap is an argument error.  8 bytes per parameter moved without acc,
 * 12 with it (28 for nabu_adam_clip_step).  NaN stays NaN, as in nabu_clip_f32. */
int nabu_clip_accumulate_f32(size_t n, float *out, const float *acc, const float *g, float clip,
                             nabu_stream_t stream);
/* The update of the last micro-batch on one replica: nabu_adam_clip_step (src = NULL, param_out updated in place) or
 * nabu_adam_clip_step_from (src read-only, no overlap with param_out) on the gradient
 *   x = clamp(grad_scale * (acc[i] + clamp(g[i], -clip, clip)), -clip, clip)
 * without the last accumulate pass and the re-read of its result: bit for bit what nabu_clip_accumulate_f32 followed
 * by nabu_adam_clip_step{,_from} on its output gives.  acc and g are read-only and do not overlap. */
int nabu_adam_clip_step_acc(size_t n, float *param_out, const float *src, const float *acc, const float *g,
                            float *m, float *v, float lr_t, float b1, float b2, float eps,
                            float clip, float grad_scale, nabu_stream_t stream);

/* Global-norm gradient clipping (the [trainer] key clip_gradient_norm; a build addition: the reference clips elements).
 * nabu_grad_norm_f32: S = sum_i x_i^2 over x = g, or x = acc + g (an fp32 add, what nabu_adam_scaled_step forms) when acc
 * is given; every term is squared and summed in double, in two launches inside the call (per-block partials into ws,
 * then one block), in an order that depends on n alone: two calls on the same data give the same bits, no atomics.
 * ws >= nabu_grad_norm_ws_bytes(n), 8-byte aligned.  g and acc are only read.  stats: four 32-bit words, 16-byte aligned:
 *   [0] float norm   = (float)((double)scale * sqrt(S))
 *   [1] float factor = norm > max_norm ? scale * (max_norm / norm) : scale   (fp32, this order; NaN when the norm is
 *                      NaN or inf) — what the update multiplies g (or acc + g) by
 *   [2] int32 skipped: incremented when the norm is NaN or inf, never cleared by the call (the caller zeroes it once)
 *   [3] 0
 * NABU_EINVAL before any launch: a null g or stats, an unaligned g / acc / stats / ws, max_norm not > 0, scale not finite
 * and > 0, acc overlapping g; NABU_EWS: a workspace that is missing or too small. */
size_t nabu_grad_norm_ws_bytes(size_t n);
int nabu_grad_norm_f32(size_t n, const float *g, const float *acc, float scale, float max_norm, float *stats,
                       void *ws, size_t ws_bytes, nabu_stream_t stream);
/* nabu_adam_clip_step{,_from,_acc} without a clamp and with grad_scale = stats[1] read on the device (stats as written
 * by nabu_grad_norm_f32 earlier on the same stream): src and acc are optional as in nabu_adam_clip_step_acc, the gradient
 * with acc is acc + g.  For a finite factor the results are, bit for bit, those of the clipping entry points called with
 * clip = +inf and grad_scale = that factor.  A NaN factor skips the update on the device: m and v keep their values and
 * so does the parameter — with src, param_out = src (after a weight-noise step param_out holds the noisy values). */
int nabu_adam_scaled_step(size_t n, float *param_out, const float *src, const float *acc, const float *g,
                          float *m, float *v, float lr_t, float b1, float b2, float eps, const float *stats,
                          nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Regularisation noise (Philox4x32-10, counter = element index, key = seed):
 *   dropout: y = x * mask / keep_prob, mask ~ Bernoulli(keep_prob) —
 *     tf.nn.dropout(x, keep_prob) in Listener/DBLSTM/Speller
 *     (models/ed_encoders/listener.py:57-59,67-69; dblstm.py:52-54).  The
 *     same (seed, offset) regenerates the mask, so the gradient is the same
 *     call applied to dy.
 *   gaussian noise: y = x + stddev * N(0,1) — input_noise
 *     (listener.py:40-45, dblstm.py:37-42). */
int nabu_dropout_f32(size_t n, const float *x, float *y, float keep_prob,
                     unsigned long long seed, unsigned long long offset,
                     nabu_stream_t stream);
int nabu_gaussian_noise_f32(size_t n, const float *x, float *y, float stddev,
                            unsigned long long seed, unsigned long long offset,
                            nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Variational weight noise of one training step (the [trainer] key weight_noise; a build addition: the reference has
 * no counterpart), ONE launch over the flat parameter buffer in 16-byte groups, n % 4 == 0:
 *   clean[e] = param[e] for every e < n;
 *   param[4 i + j] = fmaf(stddev, z[4 i + j], param[4 i + j]) for every group i inside a range of the table,
 * z = the standard normal values nabu_gaussian_noise_f32 draws for an array of n elements at (seed, offset): Philox
 * counter (i_lo, i_hi, offset_lo, offset_hi), key seed, Box-Muller — independent of the table.  A group outside every
 * range is neither stored to param nor drawn for.
 * ranges: nranges pairs [first_group, end_group) of int32 in DEVICE memory (8-byte aligned), sorted, disjoint (ranges
 *   may touch), inside [0, n / 4); ranges_host: the same table in host memory, which is what the call validates on
 *   every call (the host never reads the device copy).  nranges = 0 is legal (a copy only; both pointers may be NULL).
 * NABU_EINVAL: n % 4 != 0 or n >= 2^33, a null, unaligned (16 bytes) or overlapping param / clean, stddev negative or
 *   not finite, nranges outside 0..NABU_WEIGHT_NOISE_MAX_RANGES (the table is searched from LDS), a table that is
 *   unsorted, overlapping, empty in an entry or past the buffer. */
#define NABU_WEIGHT_NOISE_MAX_RANGES 1024
int nabu_weight_noise_f32(size_t n, float *param, float *clean, const int32_t *ranges,
                          const int32_t *ranges_host, int nranges, float stddev,
                          unsigned long long seed, unsigned long long offset, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * SpecAugment of the encoder's input features (a build addition: the reference has no counterpart): a linear time
 * warp about one random anchor frame, then time_masks time masks and freq_masks frequency masks that write zeros.
 * Out of place, one launch: x [B, T, D] batch-major, len [B] (device; a length outside 0..T is clamped), y [B, T, D].
 * Utterance b of n = len[b] frames draws Philox4x32-10 words (x, y, ., .) with key (seed_lo, seed_hi) and counter
 * (b, k, offset_lo, offset_hi); below(w, m) = ((w >> 8) * m) >> 24 in 64 bits is a uniform integer in [0, m):
 *   k = 0, only if W = time_warp > 0 and n >= 2 W + 3: anchor c = W + 1 + below(x, n - 2 W - 2) moves to
 *     c' = c - W + below(y, 2 W + 1).  Output frame t reads source position p / q = t c / c' for t < c' and
 *     (c (n-1-c') + (t-c') (n-1-c)) / (n-1-c') otherwise: i = p div q, r = p mod q (64-bit integers),
 *     out = fmaf((float)r / (float)q, in[i+1] - in[i], in[i]) when r > 0 and in[i] when r = 0 (frames 0, c', n - 1 are
 *     frames 0, c, n - 1 exactly);
 *   k = 1 + j, time mask j: t = below(x, min(time_mask_width, (int)(time_mask_ratio * (float)n)) + 1) frames from
 *     t0 = below(y, n - t + 1) become 0;
 *   k = 1 + time_masks + j, frequency mask j: with Dblk = D / feature_blocks, f = below(x, min(freq_mask_width,
 *     Dblk) + 1) columns from f0 = below(y, Dblk - f + 1) of EVERY block become 0 in the frames t < n.
 * Frames t >= n are copied.  Neither x nor y needs any alignment beyond a float's.
 * params: NULL or int32 [B, 2 + 2 time_masks + 2 freq_masks], written (c, c', t0_0, t_0, ..., f0_0, f_0, ...) per
 *   utterance ((c, c') = (0, 0) for an utterance that is not warped).
 * NABU_EINVAL: a null pointer, overlapping x and y, negative values, more than 8 masks of a kind, time_mask_ratio
 *   outside (0, 1], feature_blocks < 1 or not a divisor of D, time_warp >= 2^24.  NABU_EUNSUP: T >= 2^24 (lengths and
 *   remainders must be exact in float32), T * D >= 2^31 - 16, B > 65535. */
typedef struct nabu_specaug_desc {
  uint32_t size;            /* sizeof(nabu_specaug_desc) */
  int32_t B, T, D;
  int32_t feature_blocks;   /* equal column blocks of the feature vector (3 for static + delta + delta-delta) */
  int32_t time_warp;        /* W */
  int32_t time_masks, time_mask_width;
  int32_t freq_masks, freq_mask_width;
  float time_mask_ratio;
} nabu_specaug_desc;
int nabu_spec_augment_f32(const nabu_specaug_desc *desc, const float *x, const int32_t *len, float *y,
                          int32_t *params, unsigned long long seed, unsigned long long offset,
                          nabu_stream_t stream);

/* out[0] = scale * sum(x) (deterministic single-block tree): tf.reduce_mean of
 * the per-utterance losses (trainers/loss_functions.py:161,206-212). */
int nabu_sum_f32(size_t n, const float *x, float scale, float *out, nabu_stream_t stream);
/* y += a*x : gradient accumulation where a tensor has several consumers. */
int nabu_axpy_f32(size_t n, float a, const float *x, float *y, nabu_stream_t stream);

/* out[i] = ceil(in[i] / d): the sequence lengths after ops.pyramid_stack
 * (nabu/neuralnetworks/components/ops.py:56-58), computed where the next layer reads them
 * (a host-side recomputation + upload would synchronise the stream once per layer). */
int nabu_ceil_div_i32(int n, const int32_t *in, int d, int32_t *out, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Batch input: one packed buffer -> every padded tensor of a batch, in one launch.  Replaces the dynamic_pad of the
 * reference's batch queues (processing/input_pipeline.py:121-174, tf.train.batch / bucket_by_sequence_length) plus
 * the per-tensor feeds: the host packs the utterances WITHOUT padding, uploads the buffer with one copy and this call
 * writes each tensor padded, with its length vector.
 *
 * `packed` (device, 16-byte aligned, packed_bytes long) holds, per tensor of the batch (a segment), at byte offsets
 * the descriptor names:
 *   len_off   rows int32 lengths (4-byte aligned);
 *   row_off   rows + 1 int32 ELEMENT offsets of the rows into the segment's data: the prefix sum of len[b] * width,
 *             computed by the packer (4-byte aligned);
 *   data_off  the rows back to back, len[b] * width 4-byte elements each — float32 features or int32 labels, the
 *             kernel moves bits (16-byte aligned).
 * Result, per segment: out[b, t, :] = row b's element t for t < len[b] and 0 for len[b] <= t < max_len — EVERY element
 * of out [rows, max_len, width] is written — and out_len[b] = len[b] clamped to [0, max_len].  The clamp comes before
 * any use of the length, and a row whose offsets leave the packed buffer is written as zeros: a corrupt header cannot
 * make the kernel read or write out of bounds.  Segments with width % 4 == 0 and a 16-byte aligned out move 16 bytes per
 * lane, all others 4.
 * segs_host: nseg descriptors in HOST memory (copied into the kernel arguments; free to reuse when the call returns).
 * NABU_EINVAL before any launch: a null pointer, nseg outside 1..NABU_BATCH_MAX_SEGS, rows / width / max_len <= 0,
 * rows * max_len * width >= 2^31, a misaligned offset or pointer, an offset or extent outside packed_bytes. */
typedef struct {
  int32_t rows, width, max_len, reserved;     /* B, F (1 for label vectors), padded time extent; reserved = 0 */
  uint64_t len_off, row_off, data_off;        /* byte offsets into `packed` */
  void *out;                                  /* [rows, max_len, width] 4-byte elements */
  int32_t *out_len;                           /* [rows] */
} nabu_batch_seg;
#define NABU_BATCH_MAX_SEGS 8
int nabu_batch_unpack(int nseg, const nabu_batch_seg *segs_host, const void *packed_dev, size_t packed_bytes,
                      nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * DNNDecoder hidden layers (models/ed_decoders/dnn_decoder.py:40-51):
 * tf.contrib.layers.fully_connected = linear + ReLU, optional
 * tf.contrib.layers.layer_norm, dropout.  The linear part is nabu_gemm_f32.
 *   relu:      y = max(x, 0);  relu_bwd: dx = y > 0 ? dy : 0   (in place allowed)
 *   layer_norm (TF-1.8 contrib defaults begin_norm_axis=1, begin_params_axis=-1,
 *   variance_epsilon 1e-12): for a [B,T,F] input the moments are taken over ALL of
 *   (T,F) per batch row — padded frames included — and gamma/beta are [F]:
 *     y[b,n] = (x[b,n] - mean_b) * rstd_b * gamma[n % F] + beta[n % F],  n < N = T*F
 *   fwd saves mean[B], rstd[B]; bwd writes dx and the per-row partial sums
 *   dgamma_part/dbeta_part [B,F] (reduce them with nabu_colsum_f32; deterministic). */
int nabu_relu_f32(size_t n, const float *x, float *y, nabu_stream_t stream);
int nabu_relu_bwd_f32(size_t n, const float *y, const float *dy, float *dx, nabu_stream_t stream);
int nabu_layer_norm_fwd(int B, int N, int F, const float *x, const float *gamma, const float *beta,
                        float eps, float *y, float *mean, float *rstd, nabu_stream_t stream);
int nabu_layer_norm_bwd(int B, int N, int F, const float *x, const float *gamma, const float *dy,
                        const float *mean, const float *rstd, float *dx, float *dgamma_part,
                        float *dbeta_part, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * DNN encoder and the Kaldi-hybrid recipe (DNN/WSJ): models/ed_encoders/dnn.py:30-66,
 * components/ops.py:62-118,147-175 (stack_seq, unstack_seq, get_indices), decoders/alignment_decoder.py:32-58.
 * Frame rows of the stacked matrices lie in batch-major order: utterance b starts at row off_b = sum_{i<b} len[i],
 * computed on the device from len (the host never synchronises to learn N = sum len; it knows N from its copy).
 *
 * nabu_splice_stack_f32: splice + stack_seq in one pass.  With c = context and c' = 2c-1,
 *   out[off_b + t, j*F + f] = x[b, t + s_j, f] for t < len[b], s = (0, +1, -1, +2, -2, ..., +(c-1), -(c-1)),
 *   where a source frame outside [0, T) of the PADDED batch tensor reads 0 (dnn.py:36-44 shifts the padded tensor:
 *   frame t >= len[b] - s of utterance b reads whatever x holds there, zeros in this project's pipelines);
 *   out[r, c'F .. ld) = 0.  x [B,T,F] contiguous; out [N, ld], 16-byte aligned, ld >= c'F, ld % 4 == 0.
 * nabu_unstack_rows_f32: unstack_seq: out[b,t,:] = rows[off_b + t, :] for t < len[b], 0 for len[b] <= t < Tm
 *   (Tm = max len, not the input's T).  rows [N,H], out [B,Tm,H].
 * nabu_stack_rows_f32: its adjoint: rows[off_b + t, :] = g[b, t, :] for t < len[b].  g [B,Tm,H], rows [N,H].
 *   (both: lengths are clamped to [0, Tm]; float4 moves when H % 4 == 0 and both operands are 16-byte aligned)
 * nabu_rows_relu_ln_fwd / _bwd: tf.contrib.layers.fully_connected's ReLU followed by tf.contrib.layers.layer_norm
 *   on a 2-D input — moments PER ROW over F (unlike nabu_layer_norm_fwd's [B,T,F] semantics above):
 *     r = max(z, 0); y = (r - mean) * rstd * gamma + beta, rstd = 1/sqrt(var + eps) (var biased)
 *   fwd reads z once and writes y, mean[N], rstd[N] (of r); bwd writes dz (ReLU mask and layer-norm adjoint) and
 *   the partial sums dgamma_part/dbeta_part [P, F], P = nabu_rows_relu_ln_bwd_parts(N) (reduce them with
 *   nabu_colsum_f32; deterministic).  One wave per row.  F % 4 == 0 and F <= 4096, 16-byte aligned operands;
 *   NABU_EUNSUP for another F (the caller then runs nabu_relu_f32 + nabu_layer_norm_fwd(B = N, N = F, F), the same
 *   semantics in more launches).
 * nabu_xent_wide_loss_grad: nabu_xent_loss_grad's contract (same loss, same dlogits) for wide class counts (the
 *   3100 HMM states of DNN/WSJ): one wave per frame, an online max/sum-exp pass over the row and a second pass that
 *   writes dlogits while the row is in cache; rows t >= logit_len[b] are zero.  The per-frame terms go to ws and
 *   loss[b] is their fixed-order sum (a second, small launch): deterministic, no atomics.  Any C >= 1, any
 *   alignment (float4 body between scalar head and tail when logits and dlogits share their 16-byte phase).
 *   ws >= nabu_xent_wide_ws_bytes(B, L).
 * nabu_xent_wide_smooth_loss_grad: nabu_xent_smooth_loss_grad's contract (q = (1 - smoothing) * onehot(y) +
 *   smoothing / C; loss_t = lz - (1 - smoothing) * x_y - smoothing * mean(x); d_c = s * (softmax_c - q_c)) on the wide
 *   kernel: the row sum is accumulated in the online max/sum-exp pass from the values it loads, so it is the same two
 *   passes over the row, the same two launches, the same workspace and the same alignment rule.  smoothing outside
 *   [0, 1) or NaN: NABU_EINVAL; smoothing = 0: nabu_xent_wide_loss_grad's own instantiation, bit-identical.
 * nabu_log_softmax_prior_f32: AlignmentDecoder's pseudo log-likelihoods: out[b,t,:] = x - logsumexp(x[b,t,:]) -
 *   logprior[:] for t < len[b], 0 elsewhere; x, out [B,T,C], logprior [C].  Same row machinery as above. */
int nabu_splice_stack_f32(int B, int T, int F, int context, const float *x, const int32_t *len, float *out, int ld,
                          nabu_stream_t stream);
int nabu_unstack_rows_f32(int B, int Tm, int H, const int32_t *len, const float *rows, float *out,
                          nabu_stream_t stream);
int nabu_stack_rows_f32(int B, int Tm, int H, const int32_t *len, const float *g, float *rows, nabu_stream_t stream);
int nabu_rows_relu_ln_fwd(int N, int F, const float *z, const float *gamma, const float *beta, float eps, float *y,
                          float *mean, float *rstd, nabu_stream_t stream);
int nabu_rows_relu_ln_bwd_parts(int N);
int nabu_rows_relu_ln_bwd(int N, int F, const float *z, const float *dy, const float *gamma, const float *mean,
                          const float *rstd, float *dz, float *dgamma_part, float *dbeta_part, nabu_stream_t stream);
size_t nabu_xent_wide_ws_bytes(int B, int L);
int nabu_xent_wide_loss_grad(int B, int L, int C, int ldt, const float *logits, const int32_t *targets,
                             const int32_t *logit_len, const int32_t *target_len, float grad_scale, float *loss,
                             float *dlogits, void *ws, size_t ws_bytes, nabu_stream_t stream);
int nabu_xent_wide_smooth_loss_grad(int B, int L, int C, int ldt, const float *logits, const int32_t *targets,
                                    const int32_t *logit_len, const int32_t *target_len, float grad_scale,
                                    float smoothing, float *loss, float *dlogits, void *ws, size_t ws_bytes,
                                    nabu_stream_t stream);
int nabu_log_softmax_prior_f32(int B, int T, int C, const float *x, const int32_t *len, const float *logprior,
                               float *out, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Inference decoders — nabu/neuralnetworks/decoders.
 *
 * nabu_ctc_beam_search: CTCDecoder.__call__ (decoders/ctc_decoder.py:44-68) =
 * tf.nn.ctc_beam_search_decoder(logits, seq_len) with its defaults top_paths = 1,
 * beam_width = 100, merge_repeated = 1: CTC prefix beam search (prefix tree with per-node
 * (total, blank, label) log-probabilities, bounded beam of the beam_width best prefixes per
 * frame, blank = C-1), one workgroup per utterance over all its frames; merge_repeated also
 * collapses equal neighbours of the OUTPUT labelling, as TF's BeamEntry::LabelSeq does.
 *   logits [B,T,C] batch-major (softmax is taken inside), logit_len [B];
 *   out_ids [B,T] (entries >= out_len are -1), out_len [B], out_logprob [B] (may be NULL):
 *   log P(best prefix) under the per-frame normalised posteriors.
 * The workspace holds the prefix trees; it is initialised by the call. */
size_t nabu_ctc_beam_ws_bytes(int B, int T, int C, int beam_width);
int nabu_ctc_beam_search(int B, int T, int C, int beam_width, int merge_repeated, const float *logits,
                         const int32_t *logit_len, int32_t *out_ids, int32_t *out_len,
                         float *out_logprob, void *ws, size_t ws_bytes, nabu_stream_t stream);

/* Label n-gram language model fusion (both beam searches).  The model is a dense table of log-probabilities
 * lm_table [C^(lm_order-1), C] float32 on the device: row ctx = the previous lm_order-1 symbols as a base-C number, the
 * most recent symbol least significant; symbol C-1 is the boundary (as a context symbol the start, as a predicted
 * symbol the end of the sequence — the index of the CTC blank and of the Speller's start/end label).  The context of
 * the empty hypothesis is every digit C-1; next(ctx, c) = (ctx*C + c) mod C^(lm_order-1); lm_order 1 has one row.
 * lm_order < 1 is NABU_EINVAL, a table of more than 2^24 entries (64 MiB) NABU_EUNSUP; weights must be finite, >= 0.
 *
 * nabu_ctc_beam_search_lm: nabu_ctc_beam_search with the semantics of TensorFlow's CTC beam scorer hooks
 * (GetStateExpansionScore / GetStateEndExpansionScore), alpha = lm_weight, beta = insertion_bonus (finite):
 *   a transition that APPENDS label c to prefix g adds alpha * lm_table[ctx(g), c] + beta — the expansion candidates
 *   and the parent's contribution to a prefix already in the beam;
 *   staying in a prefix (blank, the repeated-label self loop) adds nothing;
 *   after the last frame the beam is ranked by total + alpha * lm_table[ctx, C-1], which is out_logprob.
 * merge_repeated acts on the output labelling only; the LM context is the unmerged prefix.  A tree node keeps two more
 * words (context, the term it entered with): nabu_ctc_beam_lm_ws_bytes.  With lm_weight = insertion_bonus = 0 the
 * outputs are those of nabu_ctc_beam_search, bit for bit.  The kernel is a second instantiation of the same body. */
size_t nabu_ctc_beam_lm_ws_bytes(int B, int T, int C, int beam_width);
int nabu_ctc_beam_search_lm(int B, int T, int C, int beam_width, int merge_repeated, const float *logits,
                            const int32_t *logit_len, const float *lm_table, int lm_order, float lm_weight,
                            float insertion_bonus, int32_t *out_ids, int32_t *out_len, float *out_logprob, void *ws,
                            size_t ws_bytes, nabu_stream_t stream);

/* tf.edit_distance(hyp, truth, normalize=False) per utterance (ctc_decoder.py:112-118,
 * decoders/beam_search_decoder.py:176-179): Levenshtein distance of hyp[b,:hyp_len[b]] and
 * truth[b,:truth_len[b]] (negative lengths count as 0); dist [B] int32. */
int nabu_edit_distance(int B, const int32_t *hyp, int ldh, const int32_t *hyp_len, const int32_t *truth,
                       int ldt, const int32_t *truth_len, int32_t *dist, nabu_stream_t stream);

/* Minimum word error rate training of the Speller (Prabhavalkar et al. 2018; mwer.hip, trainers/mwer.py): the expected
 * number of label errors over the N-best list of the attention beam search, plus ce_weight times the reference's
 * cross-entropy.  Rows are stacked slot-major: row n*B + b is hypothesis n of utterance b for n < N, and slot N is the
 * reference, so every slot is a block of B rows and the encoder output is tiled by repetition.
 *
 * nabu_mwer_prepare: beam output -> teacher-forcing targets.
 *   sequences [B,N,lds >= S] int32, lengths [B,N] (labels before the end label C-1, clamped to 0..S), scores [B,N]:
 *   what nabu_speller_beam_search returns; targets [B,ldr] with target_len [B], which counts the end label.
 *   stk_targets [(N+1)*B, ldt > S] (every word written): the hypothesis followed by C-1, then zeros; slot N: the first
 *     min(target_len, ldr, ldt) reference labels.  stk_len [(N+1)*B]: length + 1, the reference's clamped target_len.
 *   hyp_len [N*B]: the lengths without the end label.  valid [N*B]: 1 when the score is a real one (> -1e30; the search
 *     fills spare slots with -FLT_MAX) and no lower slot of the utterance with a real score holds the same labels
 *     [:length] (an unfinished "a b" and a finished "a b <end>" are one target).  An invalid row is the target [C-1] of
 *     length 1 with hyp_len 0.  NABU_EUNSUP: N > 16.
 * nabu_rows_tile_f32: y[r*B + b, :] = x[b, :] for r < R (x [B,F], y [R*B,F]).  nabu_rows_tile_bwd_f32: dx[b, :] =
 *   sum_r dy[r*B + b, :] in the order r = 0..R-1.  float4 accesses where an address allows, single words elsewhere: any
 *   4-byte aligned operands and any F.
 * nabu_mwer_loss_grad: logits [(N+1)*B, L, C] of the stacked targets (ldt >= L), errors [N*B] (edit distance of each
 *   hypothesis to the reference without its end label: nabu_edit_distance), valid [N*B].
 *     nll_n   = sum_{t < stk_len} (logsumexp(x[n,t,:]) - x[n,t,y_n[t]])
 *     p_n     = softmax over the valid n of -nll_n (maximum subtracted)
 *     risk[b] = sum_n p_n e_n,   nll_ref[b] = nll_N,   loss[b] = risk + ce_weight * nll_ref
 *     dlogits[n,t,:]   = -grad_scale * (p_n * sum_m p_m (e_n - e_m)) * (softmax(x[n,t,:]) - onehot(y_n[t]))
 *     dlogits[ref,t,:] =  grad_scale * ce_weight * (softmax - onehot)
 *   dlogits is exactly 0 past stk_len, on the rows of an invalid hypothesis, on all hypothesis rows when the valid
 *   error counts are equal, and on the reference rows when ce_weight == 0.  One launch, one workgroup per utterance,
 *   fixed-order sums: two calls give the same bits.  logits and dlogits must not overlap.
 *   NABU_EUNSUP (before any launch): N > 16, C < 2 or C > 1023.  NABU_EINVAL: a null pointer, B, N, L or C <= 0,
 *   ldt < L, ce_weight negative or not finite, grad_scale not finite. */
int nabu_mwer_prepare(int B, int N, int S, int lds, int C, const int32_t *sequences, const int32_t *lengths,
                      const float *scores, int ldr, const int32_t *targets, const int32_t *target_len, int ldt,
                      int32_t *stk_targets, int32_t *stk_len, int32_t *hyp_len, int32_t *valid, nabu_stream_t stream);
int nabu_rows_tile_f32(int R, int B, int F, const float *x, float *y, nabu_stream_t stream);
int nabu_rows_tile_bwd_f32(int R, int B, int F, const float *dy, float *dx, nabu_stream_t stream);
int nabu_mwer_loss_grad(int B, int N, int L, int C, int ldt, const float *logits, const int32_t *stk_targets,
                        const int32_t *stk_len, const int32_t *errors, const int32_t *valid, float ce_weight,
                        float grad_scale, float *loss, float *risk, float *nll_ref, float *dlogits,
                        nabu_stream_t stream);

/* Attention beam search — BeamSearchDecoder.__call__ (decoders/beam_search_decoder.py:31-114)
 * over components/beam_search_decoder.py:141-451 driven by dynamic_decode(maximum_iterations =
 * max_steps): the encoder output is tiled beam_width times, every step runs the Speller cell
 * (same kernels as nabu_speller_fwd) on B*beam_width rows, then
 *   nabu_beam_prune: candidates = every (beam, label) expansion plus one "stay" hypothesis per
 *     finished beam; log-softmax(logits / temperature); score = logprob / ((5+len)/6)^length_penalty;
 *     the beam_width best by score (ties: lower candidate index, as tf.nn.top_k) survive;
 *   nabu_beam_gather: survivors take the new cell state of their parent, "stay" hypotheses keep
 *     the state they had.
 * The search ends when every beam slot has been finished at some step (dynamic_decode ORs
 * `finished` over steps: the reference's decoder does not track it itself) or after max_steps.
 * Then the backwards search through the parent pointers (finalize, :341-451).
 *   values [B,Te,E] (rows >= enc_len zero), params as nabu_speller_fwd;
 *   sequences [B,W,max_steps] int32 (valid [:, :, :*num_steps]), lengths [B,W] (labels before
 *   the end token C-1), scores [B,W], alignments [B,W,max_steps,Te] or NULL.
 * SYNCHRONISES the stream once per step (the stop test) — an inference-time API.
 * Where the reference derives the parent slot of a "stay" hypothesis as idx % C (valid while
 * beam_width <= C), the slot idx - beam_width*C is used, so wider beams also work. */
typedef struct {
  uint32_t size;
  int32_t B, Te, E, U, C, num_layers;
  int32_t kind, K, F, prob_fn;        /* attention: see nabu_attn_desc */
  int32_t beam_width, max_steps;
  float length_penalty, temperature;
} nabu_beam_desc;
size_t nabu_speller_beam_ws_bytes(const nabu_beam_desc *d);
int nabu_speller_beam_search(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                             const nabu_speller_params *p, int32_t *sequences, int32_t *lengths,
                             float *scores, float *alignments, int32_t *num_steps, void *ws,
                             size_t ws_bytes, nabu_stream_t stream);
/* One pruning step on its own (testable without a model).  logits [B*W,C]; logprobs, lengths,
 * finished, seen [B,W] are updated in place; pred_ids, parent, stay [B,W] and all_seen [B] are
 * written; scratch [B, W*C+W] floats. */
int nabu_beam_prune(int B, int W, int C, const float *logits, float temperature, float length_penalty,
                    float *logprobs, int32_t *lengths, int32_t *finished, int32_t *seen,
                    int32_t *pred_ids, int32_t *parent, int32_t *stay, int32_t *all_seen,
                    float *scratch, nabu_stream_t stream);
/* One sampled step on its own (testable without a model): the sampling counterpart of nabu_beam_prune.  Row b of
 * logits [B,C] at step t draws id ~ Categorical(softmax(logits[b])) — the draw of nabu_sample_ids at prob = 1 with the
 * same seed and offset, bit for bit (Philox4x32-10, counter (b, offset), key seed; one inverse-CDF walk for both).
 *   a row not yet finished: sequences[b,t] = id; nll[b] += logsumexp(logits[b]) - logits[b,id] (fp32, max-subtracted,
 *     a fixed reduction order); with id == C-1 (the end token) or t + 1 >= max_steps: finished[b] = 1, lengths[b] = t+1;
 *   a finished row: sequences[b,t] = 0, nll[b] unchanged;
 *   every row: next_ids[b] = id (SampleEmbeddingHelper keeps feeding samples: impute_finished is off);
 *   all_finished[0] = AND of finished over the batch.
 * sequences [B,max_steps]; lengths, finished, nll [B] are updated in place; 0 <= t < max_steps. */
int nabu_sample_advance(int B, int C, const float *logits, unsigned long long seed, unsigned long long offset,
                        int t, int max_steps, int32_t *sequences, int32_t *lengths, int32_t *finished,
                        float *nll, int32_t *next_ids, int32_t *all_finished, nabu_stream_t stream);
/* Sampled decoding — RandomDecoder.__call__ (decoders/random_decoder.py:26-122): SampleEmbeddingHelper + BasicDecoder
 * under dynamic_decode(maximum_iterations = max_steps), TF-1.8 recalled.  The loop of nabu_speller_beam_search on B
 * rows (beam_width must be 1; length_penalty and temperature are ignored) with nabu_sample_advance where the search
 * prunes and gathers; step t draws at offset0 + t.  The start input is the one-hot of C-1; a row finishes at the step
 * where it draws C-1; the loop ends when every row has finished or after max_steps.
 *   sequences [B,max_steps] int32, zero beyond lengths; lengths [B] counts the end token and is max_steps for a row
 *   that never drew it; nll [B] = the summed cross-entropy of the sample (positive); alignments [B,max_steps,Te] or
 *   NULL (zero from step *num_steps on).  SYNCHRONISES the stream once per step (the stop test). */
size_t nabu_speller_sample_ws_bytes(const nabu_beam_desc *d);
int nabu_speller_sample(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                        const nabu_speller_params *p, unsigned long long seed, unsigned long long offset0,
                        int32_t *sequences, int32_t *lengths, float *nll, float *alignments, int32_t *num_steps,
                        void *ws, size_t ws_bytes, nabu_stream_t stream);
/* dst[b,w,:] = (stay[b,w] ? old : fresh)[b, parent[b,w], :]  for [B,W,F] float rows */
int nabu_beam_gather(int B, int W, int F, const float *fresh, const float *old, const int32_t *parent,
                     const int32_t *stay, float *dst, nabu_stream_t stream);

/* Joint CTC/attention beam search (Watanabe, Hori, Kim, Hershey, Hayashi 2017: hybrid CTC/attention decoding): every
 * candidate of a step also gets the CTC prefix score of the encoder's CTC head, and the beam is pruned on
 *   (1 - ctc_weight) * log p_att + ctc_weight * log p_ctc.
 * logits [B,T,C]: the head's logits on the first encoded input, enc_len [B] its lengths (clamped to 0..T); the blank
 * is C-1, which is also the Speller's end label.  y_t(k) is the log-softmax of frame t.  For a hypothesis g (its labels
 * without the start symbol, `last` its final label, -1 for the empty one) the state is r_n(t,g), r_b(t,g), t < enc_len:
 * the log-probabilities of all paths of frames 0..t that collapse to g and end in a label / in the blank, stored as
 * pairs in state [B,W,T,2]; psi [B,W] is log P_ctc(g followed by anything), 0 for the empty g.  All sums are
 * log-sum-exp in fp32; log 0 is the finite -1e30 of nabu_ctc_loss_grad, so no inf - inf arises.
 *   r_n(t, {}) = log 0, r_b(t, {}) = sum_{tau <= t} y_tau(blank);
 *   h = g.c, c != blank:  r_n(0,h) = y_0(c) if g is empty else log 0, r_b(0,h) = log 0, psi = r_n(0,h), and for t >= 1
 *     phi = r_b(t-1,g) if c == last else r_n(t-1,g) (+) r_b(t-1,g);
 *     r_n(t,h) = (r_n(t-1,h) (+) phi) + y_t(c);  r_b(t,h) = (r_b(t-1,h) (+) r_n(t-1,h)) + y_t(blank);  psi (+)= phi + y_t(c);
 *   psi(g.eos) = r_n(T-1,g) (+) r_b(T-1,g): the probability of g exactly.
 * A hypothesis that does not fit into its utterance (longer than enc_len, or repeats without room for their blanks)
 * has psi = log 0, and so has every extension of it.
 *   nabu_ctc_prefix_prepare: once per search.  Writes norm [B,T,2] (frame maximum and log of the sum of exp(x - max):
 *     y = (x - max) - log sum), and the state, psi = 0 and last = -1 of the empty hypothesis in all W slots.
 *   nabu_ctc_prefix_score: per step.  delta [B,W,C] = psi(g.c) - psi(g) for every class (c = C-1: psi(g.eos)); the row
 *     of a finished beam is zero and its state is not read.
 *   nabu_ctc_prefix_advance: per step, after pruning.  Survivor k of utterance b (parent, stay, pred as
 *     nabu_beam_prune writes them): stay -> its parent's state, psi and last; pred == C-1 -> psi(g.eos), state and last
 *     kept; otherwise the state of parent.pred, RECOMPUTED (the W*C candidate states of a step are never stored).  The
 *     new state must not overwrite the old one.
 * LDS: 4 T floats per workgroup at most; NABU_EUNSUP with a message when the device has less. */
int nabu_ctc_prefix_prepare(int B, int W, int T, int C, const float *logits, const int32_t *enc_len, float *norm,
                            float *state, float *psi, int32_t *last, nabu_stream_t stream);
int nabu_ctc_prefix_score(int B, int W, int T, int C, const float *logits, const int32_t *enc_len, const float *norm,
                          const float *state, const float *psi, const int32_t *last, const int32_t *finished,
                          float *delta, nabu_stream_t stream);
int nabu_ctc_prefix_advance(int B, int W, int T, int C, const float *logits, const int32_t *enc_len, const float *norm,
                            const float *state_in, const float *psi_in, const int32_t *last_in, const int32_t *parent,
                            const int32_t *stay, const int32_t *pred, float *state_out, float *psi_out,
                            int32_t *last_out, nabu_stream_t stream);
/* nabu_beam_prune with the CTC term: a live beam's candidate log-probability is
 *   logprobs[w] + (1 - ctc_weight) * (logits[w,c] / temperature - logsumexp) + ctc_weight * delta[w,c];
 * finished beams, "stay" candidates, the length penalty, the tie rule and every output as nabu_beam_prune (one kernel
 * body).  0 <= ctc_weight < 1; with 0 the outputs are those of nabu_beam_prune, bit for bit. */
int nabu_beam_prune_joint(int B, int W, int C, const float *logits, const float *delta, float ctc_weight,
                          float temperature, float length_penalty, float *logprobs, int32_t *lengths,
                          int32_t *finished, int32_t *seen, int32_t *pred_ids, int32_t *parent, int32_t *stay,
                          int32_t *all_seen, float *scratch, nabu_stream_t stream);
/* nabu_speller_beam_search / nabu_speller_multi_beam_search with the optional CTC operand: ctc_logits [B,Te,C] (Te of
 * the FIRST encoded input) and ctc_weight in [0, 1).  With ctc_logits NULL or ctc_weight 0 the search makes exactly the
 * launches of the plain entry point.  Otherwise: nabu_ctc_prefix_prepare before the loop, and per step
 * nabu_ctc_prefix_score before and nabu_ctc_prefix_advance after nabu_beam_prune_joint, which stands for
 * nabu_beam_prune; scores are the joint log-probabilities under the same length penalty. */
size_t nabu_speller_beam_joint_ws_bytes(const nabu_beam_desc *d);
int nabu_speller_beam_search_joint(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                   const nabu_speller_params *p, const float *ctc_logits, float ctc_weight,
                                   int32_t *sequences, int32_t *lengths, float *scores, float *alignments,
                                   int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream);
size_t nabu_speller_multi_beam_joint_ws_bytes(const nabu_multi_beam_desc *d);
int nabu_speller_multi_beam_search_joint(const nabu_multi_beam_desc *d, const float *const *values_host,
                                         const int32_t *const *enc_len_host, const nabu_speller_multi_params *p,
                                         const float *ctc_logits, float ctc_weight, int32_t *sequences,
                                         int32_t *lengths, float *scores, float *const *alignments_host,
                                         int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream);

/* nabu_beam_prune with the label n-gram term (shallow fusion, ESPnet's lm_weight) and, with delta non-NULL, the CTC
 * term of nabu_beam_prune_joint: a live beam's candidate log-probability is
 *   logprobs[w] + (1 - ctc_weight) * att + ctc_weight * delta[w,c] + lm_weight * lm_table[ctx_in[w], c]
 * (att = logits[w,c] / temperature - logsumexp; delta NULL: att alone).  Finished beams, "stay" candidates, the length
 * penalty, the tie rule and every output as nabu_beam_prune (one kernel body).  ctx_in [B,W] are the beams' contexts;
 * ctx_out [B,W] (another buffer) receives the survivors': a "stay" survivor keeps its parent's, any other gets
 * next(ctx_in[parent], pred).  With lm_weight 0 the outputs are those of nabu_beam_prune_joint (delta NULL:
 * nabu_beam_prune), bit for bit. */
int nabu_beam_prune_lm(int B, int W, int C, const float *logits, const float *delta, float ctc_weight,
                       const float *lm_table, int lm_order, float lm_weight, const int32_t *ctx_in, int32_t *ctx_out,
                       float temperature, float length_penalty, float *logprobs, int32_t *lengths, int32_t *finished,
                       int32_t *seen, int32_t *pred_ids, int32_t *parent, int32_t *stay, int32_t *all_seen,
                       float *scratch, nabu_stream_t stream);
/* The beam searches with every optional operand in one struct: the CTC operand of the *_joint entry points and the
 * label n-gram.  An operand that is NULL or has weight 0 is off, and the search then makes exactly the launches it
 * makes without it; the LM adds no launch per step (the lookup is in the prune, which also carries the contexts in a
 * double-buffered [B,W] int32 pair).  Scores are the fused log-probabilities under the same length penalty. */
typedef struct {
  uint32_t size;
  const float *ctc_logits;   /* [B,Te,C] of the first encoded input, or NULL */
  float ctc_weight;          /* in [0, 1) */
  const float *lm_table;     /* [C^(lm_order-1), C], or NULL */
  int32_t lm_order;
  float lm_weight;           /* finite, >= 0 */
} nabu_beam_search_opts;
size_t nabu_speller_beam_ex_ws_bytes(const nabu_beam_desc *d, const nabu_beam_search_opts *o);
int nabu_speller_beam_search_ex(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                const nabu_speller_params *p, const nabu_beam_search_opts *o, int32_t *sequences,
                                int32_t *lengths, float *scores, float *alignments, int32_t *num_steps, void *ws,
                                size_t ws_bytes, nabu_stream_t stream);
size_t nabu_speller_multi_beam_ex_ws_bytes(const nabu_multi_beam_desc *d, const nabu_beam_search_opts *o);
int nabu_speller_multi_beam_search_ex(const nabu_multi_beam_desc *d, const float *const *values_host,
                                      const int32_t *const *enc_len_host, const nabu_speller_multi_params *p,
                                      const nabu_beam_search_opts *o, int32_t *sequences, int32_t *lengths,
                                      float *scores, float *const *alignments_host, int32_t *num_steps, void *ws,
                                      size_t ws_bytes, nabu_stream_t stream);

/* ------------------------------------------------------------------------
 * Host-side helper of the on-disk data path (host memory, as the `_host` feature queries below):
 * CRC-32C (Castagnoli) of `n` bytes, continuing from `crc` (0 to start) — the checksum of the
 * TFRecord framing of the reference's per-utterance files.
 * Replaces: tf.python_io.TFRecordWriter / tf.TFRecordReader record checks
 * (nabu/processing/tfwriters/tfwriter.py:30-45, nabu/processing/tfreaders/tfreader.py:71-92). */
uint32_t nabu_crc32c_host(const void *data_host, size_t n, uint32_t crc);

/* ------------------------------------------------------------------------
 * Feature computation from audio: log mel filterbank (fbank) and MFCC features of a RAGGED BATCH of
 * utterances in two launches, whatever the number of utterances.
 * Replaces: nabu/processing/processors/feature_computers/{fbank,mfcc,base,sigproc}.py (numpy/scipy) and
 * the normalisation of processors/audio_processor.py:49-51.  Per utterance:
 *   snip:   num = trunc((len - winlen*rate) / (winstep*rate)); the first
 *           trunc(num*winstep*rate + winlen*rate) samples are kept (all of them if that is more);
 *   pre-emphasis on the kept samples: y[0] = s[0], y[i] = s[i] - preemph * s[i-1];
 *   frames of frame_len samples every frame_step samples, the last one zero padded, NO analysis window:
 *           one frame if kept <= frame_len, else 1 + ceil((kept - frame_len) / frame_step);
 *   power spectrum |rfft(frame, nfft)|^2 / nfft over nfft/2+1 bins; energy = sum of the bins;
 *   mel filterbank of nfilt triangles between lowfreq and highfreq (bin edges floor((nfft+1)*hz/rate));
 *           an energy or a filter output that is exactly 0 is replaced by 2^-52 before the logarithm;
 *   NABU_FEAT_FBANK: log(filter outputs); NABU_FEAT_MFCC: the first numcep coefficients of their
 *           orthonormal type-2 DCT, times 1 + (L/2) sin(pi n / L) when L = ceplifter > 0;
 *   include_energy: log(energy) is one more column behind them;
 *   dynamic 1 / 2: first (and second) derivative columns behind the static ones,
 *           d[t] = 2 x[t+2] + x[t+1] - x[t-1] - 2 x[t-2], the sequence reflected at its ends
 *           (... b a | a b c ... y z | z y ...), as often as a short utterance needs;
 *   mvn: every column minus its mean over the utterance, over its population standard deviation
 *           (two passes; a constant column divides by zero, as in the reference).
 * frame_len and frame_step must be winlen*rate and winstep*rate rounded half away from zero (the
 * rounding of the reference's Python 2).  nfft is a power of two in 256..2048 and frame_len <= nfft,
 * anything else is NABU_EUNSUP (numpy's rfft would crop the frame instead).  highfreq < 0 means rate/2.
 * Every reduction is a fixed tree inside one utterance: an utterance's features do not depend on the
 * rest of the batch.
 *
 * The host-side queries take HOST memory and touch no device:
 *   nabu_feat_num_frames   frames of an utterance of n_samples (>= 1) samples, or a negative NABU_E*;
 *   nabu_feat_plan_host    for n_utt utterances whose samples lie at sample_offsets_host[u] ..
 *                          sample_offsets_host[u+1] of one buffer: frame_offsets_host [n_utt+1] (row of
 *                          the output matrix each utterance starts at) and kept_host [n_utt] (samples
 *                          left by the snip);
 *   nabu_feat_ws_bytes     size of the table workspace (0 and a message for a bad descriptor);
 *   nabu_feat_tables_host  fills ws_host with the tables (twiddles, filter bands and weights, DCT),
 *                          computed in double precision; the caller copies them to the device once per
 *                          descriptor and passes that copy as `ws` of every nabu_feat_compute.
 * nabu_feat_compute: samples int16 (all utterances concatenated), sample_offsets / frame_offsets
 * [n_utt+1] and kept [n_utt] as planned above, max_frames = the largest frame count in the batch;
 * out [frame_offsets[n_utt], dim] float32 with dim = (nfilt or numcep, + include_energy) * (1 + dynamic). */
enum { NABU_FEAT_FBANK = 0, NABU_FEAT_MFCC = 1 };
typedef struct {
  uint32_t size;              /* sizeof(nabu_feat_desc) */
  int32_t rate;               /* samples per second */
  int32_t frame_len, frame_step;
  int32_t nfft, nfilt, numcep;
  int32_t kind;               /* NABU_FEAT_FBANK / NABU_FEAT_MFCC (numcep is ignored for fbank) */
  int32_t include_energy;     /* 0 / 1 */
  int32_t dynamic;            /* 0 nodelta, 1 delta, 2 ddelta */
  int32_t mvn;                /* 0 / 1 */
  int32_t lowfreq, highfreq;  /* Hz; highfreq < 0: rate/2 */
  float preemph, ceplifter;
  double winlen, winstep;     /* seconds (the snip works on the unrounded products with rate) */
} nabu_feat_desc;
int nabu_feat_dim(const nabu_feat_desc *d);
int nabu_feat_num_frames(const nabu_feat_desc *d, long long n_samples);
int nabu_feat_plan_host(const nabu_feat_desc *d, int n_utt, const int32_t *sample_offsets_host,
                        int32_t *frame_offsets_host, int32_t *kept_host);
size_t nabu_feat_ws_bytes(const nabu_feat_desc *d);
int nabu_feat_tables_host(const nabu_feat_desc *d, void *ws_host, size_t ws_bytes);
int nabu_feat_compute(const nabu_feat_desc *d, int n_utt, int max_frames, const int16_t *samples,
                      const int32_t *sample_offsets, const int32_t *kept, const int32_t *frame_offsets,
                      float *out, const void *ws, size_t ws_bytes, nabu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NABU_HIP_H */
