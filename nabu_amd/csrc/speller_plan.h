// speller_plan.h — the Speller's training driver (speller_train.hip): one geometry for both entry-point families and
// THE PLAN of one call.
#pragma once
#include "common.h"
#include "speller_multi.h"
#include "speller_persist.h"

namespace nabu {

// Both entry-point families as one geometry.  nabu_speller_multi_desc / _params / _grads are the general forms of
// the one-memory structs (arrays over the memories), so they ARE the normal form: nabu_speller_* fills them with M = 1.
struct SpGeo {
  bool multi;                        // the entry-point family: nabu_speller_multi_* (also with M = 1) or nabu_speller_*
  nabu_speller_multi_desc d;
  MultiAttnGeo a;                    // M, sum E, M U, column offsets; multi family: frame slices per memory, LDS
  // the call's operands (null in the size queries)
  const float *values[NABU_SPELLER_MAX_MEMORIES];
  const int32_t *enc_len[NABU_SPELLER_MAX_MEMORIES], *ids, *dec_len;
  nabu_speller_multi_params p;
  nabu_speller_multi_grads gr;       // backward pass only
  float *dvalues[NABU_SPELLER_MAX_MEMORIES];
};

// THE PLAN of one training call: which path every stage of the driver takes.  speller_plan() is the ONLY code that
// reads the driver's switches (NABU_SPELLER_STREAMS, _THREADS, _FUSED, _EPILOGUE, _ROWS16, _SPLIT, _DEFER,
// _ATTN_FUSED and the "= 2" reading of NABU_SPELLER_PERSIST) and the only caller of the predicates of
// speller_persist.hip; it is evaluated at every call (the tests flip switches inside one process) and everything else
// reads the fields.  A new kernel variant plugs in there and in the stage it replaces.  For the multi family the
// plan has one chain on the caller's stream and every fused / persistent / deferred field off.
struct SpellerPlan {
  int NS, Bn;                 // the decoder steps run as NS chains of Bn utterances on NS streams
  bool threads;               // ... each enqueued by a host thread of its own
  int S;                      // one-memory family: frame slices per utterance of the step's attention launches
  bool fused;                 // two-part products may take gemm_skinny_fused (where fused_shape() holds)
  bool tickets;               // one-memory family: the attention launches finish inside themselves (per-utterance tickets)
  bool weights_T;             // generic backward chain: products against transposed copies made once per pass (else
                              // transB products against the parameters)
  struct Pass {
    bool persist;             // the whole step loop is ONE persistent launch (speller_persist.hip)
    bool r16;                 // sub-batches of <= 16 rows: the step's products by rows16_kernel (gemm_skinny.hip)
  } fwd, bwd;
  bool cell_epi[NABU_SPELLER_MAX_LAYERS];   // forward: the LSTM cell is the epilogue of layer n's step product
  bool fuse_b, split_b;       // backward: cell as the epilogue of dq . Wq^T and ONE dz . [Kx^T | Kh^T] product; its
                              // d context half written straight into the previous step's dCtx rows
  int Sp;                     // > 0: d keys / d attention_v / d conv_proj by ONE attn_param_grads launch of Sp slices
  size_t persist_bytes;       // table + exchange rings of the persistent kernels (the larger pass); 0: no such shape
  bool persist_bwd_shape;     // ... the backward kernel's partial rows (dv8, dck8) are part of the workspace
  SpPersistDesc pd, pd_bwd;   // the persistent launches' descriptors (pd_bwd: pd without scheduled sampling, which the
                              // backward kernel and the workspace do not know of)
};

}  // namespace nabu
