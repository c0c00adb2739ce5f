// lstm_persist.h — whole-sequence persistent recurrent kernels (internal API).
#pragma once
#include "common.h"

namespace nabu {
// PACKED COMPANIONS written by the forward fp16-plane kernel next to `out` (include/nabu_hip.h, nabu_blstm_desc ABI version
// 3): the layer's output as f16x3 operands in gemm_pk.hip's layout [k / 16][plane][rows_pad][16 k] (halves of a 32-byte
// record swapped when bit 3 of the row is set), scaled by 2^14 (row maxima = the bit pattern of 1.0f).  Null pointer =
// that companion is not written.  Offsets inside one companion stay below 2^31 (checked by the caller).
struct EmitArgs {
  char *x_rows;            // out, `stack` frames per row: row = b (T / stack) + t / stack, k = (t % stack) 2H + dir H + unit
  char *x_cols;            // the transposed operand: row = that k, reduction index = that row
  char *hT[2];             // h_(t-1)^T of the forward / backward cell: row = hT_row0 + unit, reduction index = b T + t, shifted
                           // by one frame (fw: out[b, t - 1], bw: out[b, t + 1]; 0 at the ends)
  unsigned x_rows_pad, x_cols_pad, hT_rows_pad;
  int hT_row0;
  int stack_shift;         // log2(stack): 0 or 1
  int b0;                  // first batch row of this launch within the whole batch
};
// THE LAUNCH PLAN of one layer call: whether a persistent kernel runs, which family, how the batch is cut into
// launches, what workspace they need, whether the forward kernel projects its own input and whether it can write the
// companions.  lstm_persist_plan is the ONLY code that reads the NABU_PERSIST_* switches (once per process;
// NABU_PERSIST_DEBUG per call) and the device; everything else — lstm.hip, run / run_chunk — reads the fields.  A new
// kernel variant plugs in there and in run_chunk's switch over Launch::family.
enum { PERSIST_F32 = 0,     // lstm_persist.hip: exact fp32, 4 or 8 rows per unit
       PERSIST_MXH = 1,     // lstm_persist_mxh*.hip: fp16 planes, 8-row units, launches of <= 32 rows
       PERSIST_MXF = 2 };   // lstm_persist_mxf.hip: fp16 planes, 33 .. 64 rows at H = 512
struct PersistPlan {
  bool supported;                 // a persistent kernel takes this shape on this device, both passes
  int B, T, D, H, max_len;
  int ncu;                        // compute units of the device the plan was made for (at most 256)
  struct Launch { int family, rows, bs; size_t ring_bytes; };   // bs = batch rows per unit; rows = 0: no such launch
  // a pass runs the batch as consecutive launches of full.rows rows and, where B is no multiple, one of tail.rows
  struct Pass { Launch full, tail; } fwd, bwd;
  bool fuses_input;               // the forward kernel computes x_t . Wx + b itself: the caller passes x and bias and
                                  // skips its product (fp16-plane kernels: D <= 64, one launch of <= 32 rows; exact fp32:
                                  // D = 40, every launch on the 4-row geometry)
  bool emits;                     // the forward launch can write the packed companions (one PERSIST_MXH launch, every
                                  // frame visited, no debug variant)
  size_t ws_bytes, xws_bytes;     // workspace; the fp16-plane kernels' copy of x (0: input not fused there)
  size_t caller_ring_words;       // > 0 (one fp16-plane forward launch): a caller that fills something anyway may set
                                  // this many 32-bit words at the start of the workspace to 0xFFFFFFFF in that fill, on
                                  // the launch's stream, and say so (lstm_persist_fwd, ring_cleared): one launch less
};
PersistPlan lstm_persist_plan(int B, int T, int D, int H, int max_len, bool exact);   // exact: only the exact-fp32 kernels
void lstm_persist_set_timeout_us(long long us);
unsigned long long lstm_persist_timeout_ticks();   // bound of every in-kernel wait (wall_clock64 ticks)
// x, bias given (plan.fuses_input only): gates[] need NOT hold the input projection; the kernel still leaves the
// activations there.  xws: plan.xws_bytes bytes.  emit (plan.emits only): the companions to write.  x_colmax (optional,
// D words, 16-byte aligned; used where plan.xws_bytes > 0): the launch's preparation of x leaves the bit patterns of
// the columns' largest |x| there as well (it measures them for its own scale)
int lstm_persist_fwd(const PersistPlan &plan, const int32_t *len,
                     const float *const kernel[2], float *const gates[2], float *const cs[2],
                     float *out, int *status, void *ws, size_t ws_bytes, hipStream_t stream, bool ring_cleared,
                     const float *x = nullptr, const float *const bias[2] = nullptr, void *xws = nullptr,
                     const EmitArgs *emit = nullptr, uint32_t *x_colmax = nullptr);
int lstm_persist_bwd(const PersistPlan &plan, const int32_t *len,
                     const float *const kernel[2], float *const gates[2], float *const cs[2],
                     const float *dout, int *status, void *ws, size_t ws_bytes, float **db_part, int *db_rows,
                     hipStream_t stream, uint32_t *rowmax = nullptr, bool *rowmax_done = nullptr);
// rowmax (optional, [2 directions x H / 16][B T] uint32): every workgroup's largest |dz| (bit pattern) of every frame
// row over its 64 gate columns, written step by step next to dz; *rowmax_done says whether the kernels that ran keep
// it (the fp16-plane kernels of lstm_persist_mxh.hip do) — the row scales of dZ as an f16x3 operand without a pass over dz
// db_part: [db_rows][2 directions][4H] bias-gradient partial sums written by the backward kernels
// (inside ws); bias gradient of direction d = column sums of db_part[:, d, :].  In the same layout, at
// db_part + lstm_persist_db_floats(B, H): the largest |dz| of every gate column per unit (column maxima of dz = the
// maximum over the rows; the row scales of the f16x3 weight-gradient products' dZ^T operand)
size_t lstm_persist_db_floats(int B, int H);
}  // namespace nabu
