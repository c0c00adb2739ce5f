// transducer_beam.hip — one iteration of the alignment-length synchronous beam search of the RNN transducer (Saon,
// Tueske and Audhkhasi 2020) with the additive joint.  Contract: include/nabu_hip.h, nabu_transducer_beam_step.
//
// One launch per iteration, one workgroup of 256 threads per utterance.  At iteration `step` the hypothesis in a slot
// sits at frame step - out_len, so the whole beam takes one joint evaluation:
//   (1) candidates   a wave per active slot: log-sum-exp of f[b,t,:] + g_rows[b,w,:] lane-strided over C (wave_max /
//                    wave_sum), v[w,k] = score + log p(k) into LDS; NaN marks what is no candidate;
//   (2) merge        a thread per ordered pair of slots (a, c): y_a = y_c + (k), decided on the label rows themselves,
//                    adds v[c,k] to a's blank candidate and drops it.  An `a` has one partner at most and label
//                    candidates are only ever read here: no two threads touch one value;
//   (3) selection    W rounds of block_best over the candidates in LDS (decode.hip's pattern);
//   (4) placement    wave 0: a ballot splits the selected into completed hypotheses and survivors, in selection order;
//   (5) the beam     the survivors' label rows are built from the parents' rows AS FOUND, which (0) staged in LDS: a
//                    parent may feed several children and slots may permute;
//   (6) the finals   only when a hypothesis completed: a stable merge of the kept finals (copied to the workspace
//                    first) with the completed ones, both sorted already.
// Every sum runs in one fixed order and nothing is atomic: two calls give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace nabu {

constexpr int TB_NT = 256;
constexpr int TB_WMAX = 32;
constexpr int TB_NONE = INT_MIN;      // a finals slot that nothing moves into

struct BeamStepArgs {
  int T, C, S, W, step;
  const float *f, *g_rows;
  const int32_t *enc_len;
  int32_t *ids, *out_len;
  float *score;
  int32_t *parent, *emit, *last_id;
  int32_t *fin_ids, *fin_len;
  float *fin_score;
  int32_t *fin_old;                   // workspace [B][W*S]: the finals' label rows as found
};

// max + log1p(exp(min - max)); an impossible term leaves the other as it is (and never inf - inf)
__device__ __forceinline__ float tb_logadd(float p, float q) {
  const float m = fmaxf(p, q), n = fminf(p, q);
  if (n == -INFINITY) return m;
  return m + log1pf(expf(n - m));
}

__global__ __launch_bounds__(TB_NT) void transducer_beam_kernel(BeamStepArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  __shared__ Best red[2 * (TB_NT / 64)];
  __shared__ int s_len[TB_WMAX], s_flen[TB_WMAX];                                 // the beam and the finals as found
  __shared__ float s_sc[TB_WMAX], s_fsc[TB_WMAX];
  __shared__ int s_sel[TB_WMAX];                                                   // the selected, best first
  __shared__ float s_selv[TB_WMAX];
  __shared__ int s_par[TB_WMAX], s_emit[TB_WMAX], s_last[TB_WMAX], s_nlen[TB_WMAX];   // the survivors
  __shared__ float s_nsc[TB_WMAX];
  __shared__ int s_cw[TB_WMAX], s_clen[TB_WMAX], s_src[TB_WMAX];                  // the completed; who moves into a finals slot
  __shared__ float s_cv[TB_WMAX];
  __shared__ int s_na, s_nc;
  const int b = blockIdx.x, tid = threadIdx.x, W = p.W, C = p.C, S = p.S, step = p.step, blank = p.C - 1;
  const int n = W * C, rows = W * S;
  float *v = dsm;                                        // [W,C] candidates
  int *lab = reinterpret_cast<int *>(dsm + n);           // [W,S] the beam's label rows as found
  const int raw = p.enc_len[b];
  const int el = raw < 0 ? 0 : (raw > p.T ? p.T : raw);
  const size_t bw = (size_t)b * W;

  // (0) the beam as found; step 0 starts from the empty hypothesis in slot 0 whatever the state holds
  if (tid < W) {
    int len = step == 0 ? (tid == 0 ? 0 : -1) : p.out_len[bw + tid];
    const int t = step - len;
    if (len < 0 || len > S || t < 0 || t >= el) len = -1;     // empty (or no state this search leaves): nothing of it is read
    s_len[tid] = len;
    s_sc[tid] = step == 0 ? 0.f : p.score[bw + tid];
    s_flen[tid] = step == 0 ? -1 : p.fin_len[bw + tid];
    s_fsc[tid] = step == 0 ? -INFINITY : p.fin_score[bw + tid];
  }
  if (step > 0)
    for (int e = tid; e < rows; e += TB_NT) lab[e] = p.ids[bw * S + e];
  __syncthreads();

  // (1) candidates
  for (int w = tid >> 6; w < W; w += TB_NT / 64) {
    const int lane = tid & 63, len = s_len[w];
    float *vw = v + (size_t)w * C;
    if (len < 0) {
      for (int k = lane; k < C; k += 64) vw[k] = NAN;
      continue;
    }
    const float *fr = p.f + ((size_t)b * p.T + (step - len)) * C, *gr = p.g_rows + (bw + w) * C;
    float m = -INFINITY;
    for (int k = lane; k < C; k += 64) m = fmaxf(m, fr[k] + gr[k]);
    m = wave_max(m);
    float z = 0.f;
    for (int k = lane; k < C; k += 64) z += expf((fr[k] + gr[k]) - m);
    z = wave_sum(z);
    const float lz = logf(z), sc = s_sc[w];
    for (int k = lane; k < C; k += 64) vw[k] = (len < S || k == blank) ? sc + (((fr[k] + gr[k]) - m) - lz) : NAN;
  }
  __syncthreads();

  // (2) merge: y_a = y_c + (k)
  for (int pr = tid; pr < W * W; pr += TB_NT) {
    const int a = pr / W, c = pr - a * W;
    const int la = s_len[a], lc = s_len[c];
    if (la < 1 || lc < 0 || la != lc + 1) continue;
    bool same = true;
    for (int s = 0; s < lc && same; ++s) same = lab[a * S + s] == lab[c * S + s];
    const int k = lab[a * S + lc];
    if (!same || k < 0 || k >= blank) continue;
    v[a * C + blank] = tb_logadd(v[a * C + blank], v[c * C + k]);
    v[c * C + k] = NAN;
  }
  __syncthreads();

  // (3) the W best, largest first, equal values by flat index; NaN never wins
  Best mine = {-INFINITY, INT_MAX};
  for (int idx = tid; idx < n; idx += TB_NT) mine = better(mine, Best{v[idx], idx});
  int nsel = 0;
  for (int r = 0; r < W; ++r) {
    const Best g = block_best<TB_NT>(mine, red, r & 1);
    if (g.i == INT_MAX) break;                           // fewer than W candidates (the same verdict in every thread)
    if (tid == 0) {
      s_sel[r] = g.i;
      s_selv[r] = g.v;
    }
    if ((g.i % TB_NT) == tid) {
      v[g.i] = NAN;                                      // taken
      mine = Best{-INFINITY, INT_MAX};
      for (int idx = tid; idx < n; idx += TB_NT) mine = better(mine, Best{v[idx], idx});
    }
    nsel = r + 1;
  }
  __syncthreads();

  // (4) placement, in selection order: a blank on the last frame completes its hypothesis, anything else survives
  if (tid < 64) {
    const bool has = tid < nsel;
    int w = 0, k = 0;
    float val = 0.f;
    bool comp = false;
    if (has) {
      const int idx = s_sel[tid];
      w = idx / C;
      k = idx - w * C;
      val = s_selv[tid];
      comp = k == blank && (step - s_len[w]) + 1 == el;
    }
    const unsigned long long mc = __ballot(has && comp), ma = __ballot(has && !comp);
    const unsigned long long below = (1ull << tid) - 1ull;
    if (has && comp) {
      const int j = __popcll(mc & below);
      s_cw[j] = w;
      s_clen[j] = s_len[w];
      s_cv[j] = val;
    } else if (has) {
      const int j = __popcll(ma & below), e = k != blank ? 1 : 0;
      s_par[j] = w;
      s_emit[j] = e;
      s_last[j] = k;
      s_nlen[j] = s_len[w] + e;
      s_nsc[j] = val;
    }
    if (tid == 0) {
      s_na = __popcll(ma);
      s_nc = __popcll(mc);
      if (step == 0 && el == 0) {                        // no frames: the empty hypothesis is complete at once
        s_cw[0] = 0;
        s_clen[0] = 0;
        s_cv[0] = 0.f;
        s_nc = 1;
      }
    }
  }
  __syncthreads();

  // (5) the beam
  const int na = s_na, nc = s_nc;
  for (int e = tid; e < rows; e += TB_NT) {
    const int slot = e / S, s = e - slot * S;
    int val = -1;
    if (slot < na) {
      const int pw = s_par[slot], pl = s_len[pw];
      val = s < pl ? lab[pw * S + s] : (s == pl && s_emit[slot] ? s_last[slot] : -1);
    }
    p.ids[bw * S + e] = val;
  }
  if (tid < W) {
    const bool live = tid < na;
    p.out_len[bw + tid] = live ? s_nlen[tid] : -1;
    p.score[bw + tid] = live ? s_nsc[tid] : -INFINITY;
    p.parent[bw + tid] = live ? s_par[tid] : tid;
    p.emit[bw + tid] = live ? s_emit[tid] : 0;
    p.last_id[bw + tid] = live ? s_last[tid] : blank;
  }

  // (6) the finals: kept ones first among equal scores, what falls past W is dropped
  if (nc == 0 && step > 0) return;
  int nf = 0;
  for (int j = 0; j < W; ++j) nf += s_flen[j] >= 0 ? 1 : 0;           // (they sit in slots 0 .. nf-1)
  int32_t *old = p.fin_old + bw * S;
  if (nf)
    for (int e = tid; e < rows; e += TB_NT) old[e] = p.fin_ids[bw * S + e];
  if (tid < W) s_src[tid] = TB_NONE;
  __syncthreads();
  if (tid < nf) {
    int pos = tid;
    for (int m = 0; m < nc; ++m) pos += s_cv[m] > s_fsc[tid] ? 1 : 0;
    if (pos < W) s_src[pos] = tid;
  } else if (tid >= 64 && tid - 64 < nc) {
    const int m = tid - 64;
    int pos = m;
    for (int j = 0; j < nf; ++j) pos += s_fsc[j] >= s_cv[m] ? 1 : 0;
    if (pos < W) s_src[pos] = -1 - m;
  }
  __syncthreads();
  for (int e = tid; e < rows; e += TB_NT) {
    const int pos = e / S, s = e - pos * S, src = s_src[pos];
    int val = -1;
    if (src >= 0) val = old[src * S + s];
    else if (src != TB_NONE && s < s_clen[-1 - src]) val = lab[s_cw[-1 - src] * S + s];
    p.fin_ids[bw * S + e] = val;
  }
  if (tid < W) {
    const int src = s_src[tid];
    p.fin_len[bw + tid] = src >= 0 ? s_flen[src] : (src != TB_NONE ? s_clen[-1 - src] : -1);
    p.fin_score[bw + tid] = src >= 0 ? s_fsc[src] : (src != TB_NONE ? s_cv[-1 - src] : -INFINITY);
  }
}

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_transducer_beam_ws_bytes(int B, int W, int C, int S) {
  if (B <= 0 || W <= 0 || C <= 0 || S <= 0) return 0;
  return align_up((size_t)B * W * S * sizeof(int32_t), 16);
}

extern "C" int nabu_transducer_beam_step(int B, int T, int C, int S, int W, int step, const float *f, const float *g_rows,
                                         const int32_t *enc_len, int32_t *ids, int32_t *out_len, float *score,
                                         int32_t *parent, int32_t *emit, int32_t *last_id, int32_t *fin_ids,
                                         int32_t *fin_len, float *fin_score, void *ws, size_t ws_bytes,
                                         nabu_stream_t stream) {
  NABU_CHECK_ARG(W >= 1 && W <= TB_WMAX, "transducer_beam_step: W=%d outside 1..%d", W, TB_WMAX);
  NABU_CHECK_ARG(B >= 1 && B <= 65535, "transducer_beam_step: B=%d outside 1..65535", B);
  NABU_CHECK_ARG(T >= 1, "transducer_beam_step: T=%d < 1", T);
  NABU_CHECK_ARG(S >= 1, "transducer_beam_step: S=%d < 1", S);
  NABU_CHECK_ARG(C >= 2, "transducer_beam_step: C=%d < 2", C);
  NABU_CHECK_ARG(step >= 0, "transducer_beam_step: step=%d < 0", step);
  NABU_CHECK_ARG(f && g_rows && enc_len, "transducer_beam_step: null pointer among f, g_rows, enc_len");
  NABU_CHECK_ARG(ids && out_len && score, "transducer_beam_step: null pointer among ids, out_len, score");
  NABU_CHECK_ARG(parent && emit && last_id, "transducer_beam_step: null pointer among parent, emit, last_id");
  NABU_CHECK_ARG(fin_ids && fin_len && fin_score, "transducer_beam_step: null pointer among fin_ids, fin_len, fin_score");
  NABU_CHECK_ARG(ws, "transducer_beam_step: null pointer ws");
  const size_t need = nabu_transducer_beam_ws_bytes(B, W, C, S);
  if (ws_bytes < need) return fail(NABU_EWS, "transducer_beam_step: workspace ws_bytes %zu < %zu", ws_bytes, need);
  const size_t lds = ((size_t)W * C + (size_t)W * S) * sizeof(float);      // more than a CU has: NABU_EUNSUP
  BeamStepArgs p;
  p.T = T; p.C = C; p.S = S; p.W = W; p.step = step;
  p.f = f; p.g_rows = g_rows; p.enc_len = enc_len;
  p.ids = ids; p.out_len = out_len; p.score = score;
  p.parent = parent; p.emit = emit; p.last_id = last_id;
  p.fin_ids = fin_ids; p.fin_len = fin_len; p.fin_score = fin_score;
  p.fin_old = static_cast<int32_t *>(ws);
  return launch_lds(transducer_beam_kernel, dim3(B), dim3(TB_NT), lds, static_cast<hipStream_t>(stream), p);
}
