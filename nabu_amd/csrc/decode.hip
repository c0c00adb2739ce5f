// decode.hip — inference decoders: CTC prefix beam search, the attention
// beam search of the reference's BeamSearchDecoder, and the edit distance both evaluate with.
//
// These are latency-bound integer/control kernels, not bandwidth kernels: a decoding step handles
// a few thousand candidates per utterance.  The design goal is that nothing leaves the device
// between the model's forward pass and the decoded label sequences:
//   * CTC: ONE launch for the whole batch; a workgroup owns an utterance, walks its frames and
//     keeps the beam (<= beam_width prefixes with their blank/label/total log-probabilities) in
//     LDS; the prefix tree (parent, label, beam slot, children table) lives in an HBM workspace
//     that stays L2-resident.
//   * attention: the per-step cell kernels of speller.hip / speller_multi.hip on B*beam_width rows, then one
//     pruning workgroup per utterance and row gathers of the cell state (ONE loop for 1..M encoded inputs: beam_run).
//     The sampled decode (the reference's RandomDecoder) is a mode of that loop: beam_width 1, and one wave per row
//     draws the next label (sample_advance_kernel) where the beam search prunes and gathers.
// Selecting the k best of n candidates, exact and deterministic with ties to the lower candidate
// index: CTC (k = 100 of ~4000 per frame) uses a radix select of the k-th largest key + compaction +
// rank sort (select_best); the attention search (k = 16) uses k rounds of a workgroup-wide arg-max
// in which every thread caches the best of its own strided share and only the owner of the removed
// candidate rescans.
#include <float.h>
#include <limits.h>

#include <type_traits>
#include <vector>

#include "common.h"
#include "speller_multi.h"

namespace nabu {

constexpr int DT = 256;  // threads per workgroup of the decoding kernels

__device__ __forceinline__ float lse2d(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const float m = fmaxf(a, b), n = fminf(a, b);
  return m + log1pf(expf(n - m));
}

// order-preserving map float -> uint32 (larger float = larger integer); -inf and NaN map to 0 = "dead"
__device__ __forceinline__ unsigned key_image(float x) {
  if (!(x > -INFINITY)) return 0u;
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The `want` best of keys[0..n) by (value desc, index asc), dead keys (-inf/NaN) never: writes their
// indices best-first to sel[] and returns how many there are (uniform).  One barrier-synchronised
// routine for the whole workgroup; scratch: hist[256], list_u/list_i[want], ties[n], sc[8].
__device__ __forceinline__ int select_best(const float *keys, int n, int want, int *hist, unsigned *list_u, int *list_i,
                           int *ties, int *sel, int *sc) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0;
  int need = want;             // rank of the threshold key among the keys matching the prefix so far
  bool all_live = false;       // fewer live keys than `want`: take them all
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? (0xFFFFFFFFu << (shift + 8)) : 0u;
    for (int i = tid; i < 256; i += DT) hist[i] = 0;
    __syncthreads();
    for (int idx = tid; idx < n; idx += DT) {
      const unsigned u = key_image(keys[idx]);
      if (u && (u & himask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid < 64) {
      const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const int s4 = h0 + h1 + h2 + h3;
      int inc = s4;                                  // inclusive suffix sum over lanes >= this one
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(inc, o);
        if (lane + o < 64) inc += t;
      }
      if (lane == 0) sc[2] = inc;                    // keys matching the prefix
      int a = inc - s4;                              // keys in higher bins
      const int hh[4] = {h0, h1, h2, h3};
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (a < need && need <= a + hh[b]) { sc[0] = 4 * lane + b; sc[1] = need - a; }
        a += hh[b];
      }
    }
    __syncthreads();
    if (sc[2] < need) { all_live = true; break; }    // only possible in pass 0 (uniform)
    prefix |= (unsigned)sc[0] << shift;
    need = sc[1];
    __syncthreads();
  }
  // compaction
  if (tid == 0) { sc[3] = 0; sc[4] = 0; }
  __syncthreads();
  const unsigned thr = all_live ? 0u : prefix;
  for (int idx = tid; idx < n; idx += DT) {
    const unsigned u = key_image(keys[idx]);
    if (!u) continue;
    if (u > thr) {
      const int pos = atomicAdd(&sc[3], 1);
      list_u[pos] = u; list_i[pos] = idx;
    } else if (u == thr) {
      ties[atomicAdd(&sc[4], 1)] = idx;
    }
  }
  __syncthreads();
  const int above = sc[3], nties = all_live ? 0 : sc[4];
  // of the keys equal to the threshold the `need` lowest indices survive
  for (int t = tid; t < nties; t += DT) {
    const int me = ties[t];
    int rank = 0;
    if (nties > need)
      for (int j = 0; j < nties; ++j) rank += ties[j] < me;
    else
      rank = 0;
    if (nties <= need || rank < need) {
      const int pos = atomicAdd(&sc[3], 1);
      list_u[pos] = thr; list_i[pos] = me;
    }
  }
  __syncthreads();
  const int m = sc[3];
  (void)above;
  // rank sort (keys descending, equal keys by ascending index)
  for (int t = tid; t < m; t += DT) {
    const unsigned u = list_u[t];
    const int i = list_i[t];
    int rank = 0;
    for (int j = 0; j < m; ++j) {
      const unsigned uj = list_u[j];
      rank += (uj > u) || (uj == u && list_i[j] < i);
    }
    sel[rank] = i;
  }
  __syncthreads();
  return m;
}

// ===========================================================================
// CTC prefix beam search
struct CtcBeamArgs {
  int B, T, C, W, merge, NN;
  const float *logits;
  const int32_t *len;
  int32_t *out_ids, *out_len;
  float *out_lp;
  int32_t *nodes;   // per utterance: parent[NN], label[NN], slot[NN], children[NN*(C-1)]; LM: then ctx[NN], term[NN]
  size_t per_utt;   // int32 words per utterance
};
// LM: the label n-gram table [nctx, C] (log-probabilities), nctx = C^(order-1) contexts, and its weights.  The plain
// instantiation takes CtcBeamArgs as it always did.
struct CtcBeamLmArgs : CtcBeamArgs {
  const float *lm;
  int nctx;
  float alpha, beta;
};
template <bool LM> using CtcArgs = std::conditional_t<LM, CtcBeamLmArgs, CtcBeamArgs>;

// the context after label c: the previous order-1 symbols as a base-C number, the most recent least significant
__device__ __forceinline__ int lm_next(int ctx, int c, int C, int nctx) { return (ctx * C + c) % nctx; }

// LM: label n-gram fusion with the semantics of TF's scorer hooks (nabu_ctc_beam_search_lm).  A transition that APPENDS
// label c to prefix g carries alpha * lm[ctx(g), c] + beta — the expansion candidates of (2) and the parent's
// contribution to a leaf in (1) —, staying in a prefix (blank, the repeated-label self loop) carries nothing.  A node
// keeps its context and the term it entered with; after the last frame the leaves are ranked with the end term.
template <bool LM>
__global__ __launch_bounds__(DT) void ctc_beam_kernel(CtcArgs<LM> p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  __shared__ int s_nl, s_nnodes;
  const int b = blockIdx.x, tid = threadIdx.x, W = p.W, C = p.C, C1 = p.C - 1, blank = p.C - 1;
  float *inp = dsm;                                 // [C]   log-softmax of the frame
  float *s_tot = inp + C;                           // [W]   newp of the leaves, best first
  float *s_blk = s_tot + W, *s_lab = s_blk + W;
  float *o_tot = s_lab + W, *o_blk = o_tot + W;     // [W]   oldp
  float *n_tot = o_blk + W, *n_blk = n_tot + W, *n_lab = n_blk + W;
  int *s_node = reinterpret_cast<int *>(n_lab + W); // [W]   tree node of a beam slot
  int *s_lbl = s_node + W, *n_node = s_lbl + W, *n_lbl = n_node + W, *sel = n_lbl + W;
  float *keys = reinterpret_cast<float *>(sel + W); // [W*C] selection keys: leaves, then expansions
  int *ties = reinterpret_cast<int *>(keys + W * C);   // [W*C] candidates equal to the W-th key
  unsigned *list_u = reinterpret_cast<unsigned *>(ties + W * C);   // [W] survivors: key image, index
  int *list_i = reinterpret_cast<int *>(list_u + W);
  int *hist = list_i + W;                              // [256]
  __shared__ int s_sc[8];
  int32_t *parent = p.nodes + (size_t)b * p.per_utt, *label = parent + p.NN, *slot = label + p.NN,
          *child = slot + p.NN;
  [[maybe_unused]] int32_t *nctx = child + (size_t)p.NN * C1;                  // LM only: context index of a node,
  [[maybe_unused]] float *nterm = reinterpret_cast<float *>(nctx + p.NN);      //          the term it entered with
  int Tb = p.len[b];
  Tb = Tb < 0 ? 0 : (Tb > p.T ? p.T : Tb);
  if (tid == 0) {
    // the root: P(empty prefix) = 1, all of it "ending in blank"
    parent[0] = -1; label[0] = -1; slot[0] = 0;
    s_node[0] = 0; s_lbl[0] = -1;
    s_tot[0] = 0.f; s_blk[0] = 0.f; s_lab[0] = -INFINITY;
    s_nl = 1; s_nnodes = 1;
    if constexpr (LM) nctx[0] = p.nctx - 1;         // the empty hypothesis: every digit the boundary C-1
  }
  __syncthreads();
  const float *lg = p.logits + (size_t)b * p.T * C;
  for (int t = 0; t < Tb; ++t) {
    const int nl = s_nl;
    if (nl == 0) break;
    if (tid < 64) {
      const float *x = lg + (size_t)t * C;
      float m = -INFINITY;
      for (int c = tid; c < C; c += 64) m = fmaxf(m, x[c]);
      m = wave_max(m);
      float s = 0.f;
      for (int c = tid; c < C; c += 64) s += expf(x[c] - m);
      const float lz = m + logf(wave_sum(s));
      for (int c = tid; c < C; c += 64) inp[c] = x[c] - lz;
    }
    __syncthreads();
    // (1) the leaves: P(prefix @t) from P(prefix @t-1) and from the parent prefix
    float ot = 0.f, ob = 0.f, nt = 0.f, nb = 0.f, nlb = 0.f;
    if (tid < nl) {
      ot = s_tot[tid]; ob = s_blk[tid];
      nlb = s_lab[tid];
      const int node = s_node[tid], par = parent[node], lab = s_lbl[tid];
      if (par >= 0) {
        const int ps = slot[par];
        if constexpr (LM) {
          if (ps >= 0) nlb = lse2d(nlb, (lab == s_lbl[ps] ? s_blk[ps] : s_tot[ps]) + nterm[node]);
        } else {
          if (ps >= 0) nlb = lse2d(nlb, lab == s_lbl[ps] ? s_blk[ps] : s_tot[ps]);   // parent still in the beam
        }
        nlb += inp[lab];
      }
      nb = ot + inp[blank];
      nt = lse2d(nb, nlb);
    }
    __syncthreads();
    if (tid < nl) {
      o_tot[tid] = ot; o_blk[tid] = ob;
      s_tot[tid] = nt; s_blk[tid] = nb; s_lab[tid] = nlb;
      keys[tid] = nt;
    }
    __syncthreads();
    // (2) expansions by one label of every leaf whose child is not itself a leaf
    const int ncand = nl * C1, n = nl + ncand;
    for (int idx = tid; idx < ncand; idx += DT) {
      const int i = idx / C1, c = idx - i * C1;
      const int ch = child[(size_t)s_node[i] * C1 + c];
      float sc = -INFINITY;
      if constexpr (LM) {
        if (!(ch >= 0 && slot[ch] >= 0) && o_tot[i] > -INFINITY)
          sc = inp[c] + ((c == s_lbl[i] ? o_blk[i] : o_tot[i]) +
                         __fmaf_rn(p.alpha, p.lm[(size_t)nctx[s_node[i]] * C + c], p.beta));
      } else {
        if (!(ch >= 0 && slot[ch] >= 0) && o_tot[i] > -INFINITY) sc = inp[c] + (c == s_lbl[i] ? o_blk[i] : o_tot[i]);
      }
      keys[nl + idx] = sc;
    }
    __syncthreads();
    // (3) the beam_width best: radix select of the W-th largest key (4 passes over 8-bit digits of
    // the order-preserving integer image of the floats, 256-bin histograms in LDS), compaction of
    // everything above it plus the lowest-index ties, then a rank sort of the <= W survivors
    const int nsel = select_best(keys, n, W, hist, list_u, list_i, ties, sel, s_sc);
    // (4) the new beam, best first; prefixes entering the tree get a node
    if (tid < nl) slot[s_node[tid]] = -1;
    __syncthreads();
    if (tid < nsel) {
      const int g = sel[tid];
      if (g < nl) {
        n_node[tid] = s_node[g]; n_lbl[tid] = s_lbl[g];
        n_tot[tid] = s_tot[g]; n_blk[tid] = s_blk[g]; n_lab[tid] = s_lab[g];
      } else {
        const int idx = g - nl, i = idx / C1, c = idx - i * C1;
        int32_t *cp = child + (size_t)s_node[i] * C1 + c;
        int ch = *cp;
        [[maybe_unused]] float term = 0.f;
        if constexpr (LM) term = __fmaf_rn(p.alpha, p.lm[(size_t)nctx[s_node[i]] * C + c], p.beta);
        if (ch < 0) {
          ch = atomicAdd(&s_nnodes, 1);
          *cp = ch;
          parent[ch] = s_node[i];
          label[ch] = c;
          if constexpr (LM) { nctx[ch] = lm_next(nctx[s_node[i]], c, C, p.nctx); nterm[ch] = term; }
        }
        float sc = inp[c] + (c == s_lbl[i] ? o_blk[i] : o_tot[i]);
        if constexpr (LM) sc = inp[c] + ((c == s_lbl[i] ? o_blk[i] : o_tot[i]) + term);
        n_node[tid] = ch; n_lbl[tid] = c;
        n_tot[tid] = sc; n_lab[tid] = sc; n_blk[tid] = -INFINITY;
      }
    }
    __syncthreads();
    if (tid < nsel) {
      s_node[tid] = n_node[tid]; s_lbl[tid] = n_lbl[tid];
      s_tot[tid] = n_tot[tid]; s_blk[tid] = n_blk[tid]; s_lab[tid] = n_lab[tid];
      slot[n_node[tid]] = tid;
    }
    if (tid == 0) s_nl = nsel;
    __syncthreads();
  }
  // the labelling of the best leaf (BeamEntry::LabelSeq): walk to the root
  __shared__ int s_len;
  [[maybe_unused]] int top = 0;                     // the slot of the best leaf
  [[maybe_unused]] float top_lp = -INFINITY;
  if constexpr (LM) {
    if (s_nl > 0) {
      // rank the leaves once more with the end term (GetStateEndExpansionScore); ties to the better slot
      __shared__ Best s_red[2 * (DT / 64)];
      Best mine = {-INFINITY, INT_MAX};
      if (tid < s_nl) mine = Best{s_tot[tid] + p.alpha * p.lm[(size_t)nctx[s_node[tid]] * C + blank], tid};
      const Best g = block_best<DT>(mine, s_red, 0);
      top_lp = s_tot[0];
      if (g.i != INT_MAX) { top = g.i; top_lp = g.v; }
    }
  }
  if (tid == 0) {
    int n = 0;
    if (s_nl > 0) {
      int prev = -1;
      for (int x = s_node[LM ? top : 0]; x > 0; x = parent[x]) {
        const int l = label[x];
        if (!p.merge || l != prev) ++n;
        prev = l;
      }
      int k = n;
      prev = -1;
      for (int x = s_node[LM ? top : 0]; x > 0; x = parent[x]) {
        const int l = label[x];
        if (!p.merge || l != prev) p.out_ids[(size_t)b * p.T + --k] = l;
        prev = l;
      }
    }
    p.out_len[b] = n;
    if constexpr (LM) {
      if (p.out_lp) p.out_lp[b] = top_lp;
    } else {
      if (p.out_lp) p.out_lp[b] = s_nl > 0 ? s_tot[0] : -INFINITY;
    }
    s_len = n;
  }
  __syncthreads();
  for (int k = s_len + tid; k < p.T; k += DT) p.out_ids[(size_t)b * p.T + k] = -1;
}

static size_t ctc_beam_lds(int C, int W) { return ((size_t)C + 15 * (size_t)W + 2 * (size_t)W * C + 256) * 4; }

// ===========================================================================
// Levenshtein distance, one workgroup per pair, anti-diagonal wavefront in LDS
__global__ __launch_bounds__(DT) void edit_distance_kernel(int B, const int32_t *__restrict__ hyp, int ldh,
                                                           const int32_t *__restrict__ hyp_len,
                                                           const int32_t *__restrict__ truth, int ldt,
                                                           const int32_t *__restrict__ truth_len,
                                                           int32_t *__restrict__ dist) {
  extern __shared__ int ism[];
  const int b = blockIdx.x, tid = threadIdx.x;
  int n = hyp_len[b], m = truth_len[b];
  n = n < 0 ? 0 : (n > ldh ? ldh : n);
  m = m < 0 ? 0 : (m > ldt ? ldt : m);
  int *d2 = ism, *d1 = d2 + ldh + 1, *d0 = d1 + ldh + 1;
  const int32_t *h = hyp + (size_t)b * ldh, *r = truth + (size_t)b * ldt;
  // diagonal k holds D[i][k-i] at index i
  for (int k = 0; k <= n + m; ++k) {
    const int lo = k - m > 0 ? k - m : 0, hi = k < n ? k : n;
    for (int i = lo + tid; i <= hi; i += DT) {
      const int j = k - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else {
        v = min(d1[i - 1], d1[i]) + 1;
        v = min(v, d2[i - 1] + (h[i - 1] != r[j - 1] ? 1 : 0));
      }
      d0[i] = v;
    }
    __syncthreads();
    int *tmp = d2; d2 = d1; d1 = d0; d0 = tmp;
  }
  if (tid == 0) dist[b] = d1[n];
}

// ===========================================================================
// attention beam search: pruning, state gather, backwards search
struct PruneArgs {
  int B, W, C;
  const float *logits;
  float inv_temp, lpw;
  float *logprobs;
  int32_t *lengths, *finished, *seen, *pred, *parent, *stay, *all_seen;
  float *scratch;
  const float *delta;      // JOINT: [B,W,C] CTC prefix score differences (ctc_prefix.hip), and their weight
  float ctcw;
};
// LM: the label n-gram table [nctx, C], its weight, and the beams' contexts [B,W] before / after.  The instantiations
// without the LM take PruneArgs as they always did.
struct PruneLmArgs : PruneArgs {
  const float *lm;
  int nctx;
  float lmw;
  const int32_t *ctx_in;
  int32_t *ctx_out;
};
template <bool LM> using PruneArgsOf = std::conditional_t<LM, PruneLmArgs, PruneArgs>;

__device__ __forceinline__ float length_penalty(int len, float w, float pen6) {
  return w == 0.f ? 1.f : powf(5.f + (float)len, w) / pen6;
}

// JOINT: a live beam's candidate adds (1 - ctcw) * attention log-probability + ctcw * delta instead of the
// attention log-probability (nabu_beam_prune_joint); everything else is the one body
// LM: a live beam's candidate also adds lmw * lm[ctx[w], c] (shallow fusion, nabu_beam_prune_lm), and the survivors'
// contexts are written: a "stay" survivor keeps its parent's, any other gets lm_next(ctx[parent], pred)
template <bool JOINT, bool LM>
__global__ __launch_bounds__(DT) void beam_prune_kernel(PruneArgsOf<LM> p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  __shared__ Best red[2 * (DT / 64)];
  __shared__ int s_all;
  const int b = blockIdx.x, tid = threadIdx.x, W = p.W, C = p.C, end = p.C - 1;
  const int n = W * C + W;
  float *lz = dsm, *plp = lz + W;
  int *plen = reinterpret_cast<int *>(plp + W), *pfin = plen + W, *sel = pfin + W;
  [[maybe_unused]] int *pctx = sel + W;                 // LM only
  float *sc = p.scratch + (size_t)b * n;
  const float *lg = p.logits + (size_t)b * W * C;
  for (int w = tid >> 6; w < W; w += DT / 64) {
    const float *x = lg + (size_t)w * C;
    const int l = tid & 63;
    float m = -INFINITY;
    for (int c = l; c < C; c += 64) m = fmaxf(m, x[c] * p.inv_temp);
    m = wave_max(m);
    float s = 0.f;
    for (int c = l; c < C; c += 64) s += expf(x[c] * p.inv_temp - m);
    s = wave_sum(s);
    if (l == 0) lz[w] = m + logf(s);
  }
  for (int w = tid; w < W; w += DT) {
    plp[w] = p.logprobs[(size_t)b * W + w];
    plen[w] = p.lengths[(size_t)b * W + w];
    pfin[w] = p.finished[(size_t)b * W + w];
    if constexpr (LM) pctx[w] = min(max(p.ctx_in[(size_t)b * W + w], 0), p.nctx - 1);     // (a table row, whatever the caller wrote)
  }
  if (tid == 0) s_all = 1;
  __syncthreads();
  const float pen6 = powf(6.f, p.lpw);
  auto candidate = [&](int idx, float &lp, int &len, int &id) {
    if (idx < W * C) {
      const int w = idx / C, c = idx - w * C;
      float nl = pfin[w] ? -FLT_MAX : lg[idx] * p.inv_temp - lz[w];
      if (JOINT && !pfin[w]) nl = (1.f - p.ctcw) * nl + p.ctcw * p.delta[(size_t)b * W * C + idx];
      if constexpr (LM) {
        if (!pfin[w]) nl = __fmaf_rn(p.lmw, p.lm[(size_t)pctx[w] * C + c], nl);
      }
      lp = plp[w] + nl;
      len = plen[w] + (c != end ? 1 : 0);
      id = c;
    } else {
      const int j = idx - W * C;
      lp = pfin[j] ? plp[j] : -FLT_MAX;
      len = plen[j];
      id = end;
    }
  };
  for (int idx = tid; idx < n; idx += DT) {
    float lp; int len, id;
    candidate(idx, lp, len, id);
    sc[idx] = lp / length_penalty(len, p.lpw, pen6);
  }
  __syncthreads();
  Best mine = {-INFINITY, INT_MAX};
  for (int idx = tid; idx < n; idx += DT) mine = better(mine, Best{sc[idx], idx});
  for (int k = 0; k < W; ++k) {
    Best g = block_best<DT>(mine, red, k & 1);
    if (g.i == INT_MAX) g.i = k;                         // only NaNs left (NaN logits): any slot
    if (tid == 0) sel[k] = g.i;
    if ((g.i % DT) == tid) {
      sc[g.i] = NAN;                                      // taken; -inf scores stay selectable (tf.nn.top_k)
      mine = Best{-INFINITY, INT_MAX};
      for (int idx = tid; idx < n; idx += DT) mine = better(mine, Best{sc[idx], idx});
    }
  }
  __syncthreads();
  for (int k = tid; k < W; k += DT) {
    const int g = sel[k];
    float lp; int len, id;
    candidate(g, lp, len, id);
    const size_t o = (size_t)b * W + k;
    const int st = g >= W * C;
    p.parent[o] = st ? g - W * C : g / C;
    if constexpr (LM) p.ctx_out[o] = st ? pctx[g - W * C] : lm_next(pctx[g / C], id, C, p.nctx);
    p.stay[o] = st;
    p.pred[o] = id;
    p.logprobs[o] = lp;
    p.lengths[o] = len;
    const int fin = id == end;
    p.finished[o] = fin;
    const int sn = p.seen[o] | fin;
    p.seen[o] = sn;
    if (!sn) s_all = 0;
  }
  __syncthreads();
  if (tid == 0) p.all_seen[b] = s_all;
}

// ===========================================================================
// sampled decoding: one step of SampleEmbeddingHelper + BasicDecoder under dynamic_decode.  One wave per row; the logits
// are read once (into LDS up to SAMPLE_LDS_C classes; wider rows are walked in place).  The wave reduces the row's
// log-sum-exp (strided partials, then the xor butterfly: a fixed order); lane 0 draws with softmax_draw — the walk and
// the Philox word of nabu_sample_ids at prob = 1 — and does the row's bookkeeping.
constexpr int SAMPLE_LDS_C = 4096;
struct SampleArgs {
  int C, t, max_steps;
  const float *logits;
  unsigned long long seed, offset;
  int32_t *sequences, *lengths, *finished, *next_ids, *all_finished;
  float *nll;
};

__global__ __launch_bounds__(64) void sample_advance_kernel(SampleArgs p) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int b = blockIdx.x, lane = threadIdx.x, C = p.C;
  const float *x = p.logits + (size_t)b * C;
  const bool staged = C <= SAMPLE_LDS_C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    const float v = x[c];
    if (staged) dsm[c] = v;
    m = fmaxf(m, v);
  }
  m = wave_max(m);
  __syncthreads();
  const float *l = staged ? dsm : x;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(l[c] - m);
  s = wave_sum(s);
  if (lane) return;
  const uint4 r = philox4x32_10(make_uint4((unsigned)b, 0u, (unsigned)p.offset, (unsigned)(p.offset >> 32)),
                                make_uint2((unsigned)p.seed, (unsigned)(p.seed >> 32)));
  const int id = softmax_draw(l, C, u01(r.y));
  p.next_ids[b] = id;                  // fed to the cell also after the end token (impute_finished is off)
  int32_t *out = p.sequences + (size_t)b * p.max_steps + p.t;
  if (p.finished[b]) { *out = 0; return; }
  *out = id;
  p.nll[b] += logf(s) + (m - l[id]);     // logsumexp - logit, the two large terms subtracted first
  if (id == C - 1 || p.t + 1 >= p.max_steps) {
    p.finished[b] = 1;
    p.lengths[b] = p.t + 1;
  } else {
    atomicAnd(p.all_finished, 0);      // (set to 1 before the launch: the AND of `finished` over the batch)
  }
}

__global__ __launch_bounds__(DT) void beam_gather_kernel(int W, int F, const float *__restrict__ fresh,
                                                         const float *__restrict__ old,
                                                         const int32_t *__restrict__ parent,
                                                         const int32_t *__restrict__ stay,
                                                         float *__restrict__ dst) {
  const int row = blockIdx.x, b = row / W;
  const float *src = (stay[row] ? old : fresh) + ((size_t)b * W + parent[row]) * F;
  float *d = dst + (size_t)row * F;
  for (int f = blockIdx.y * DT + threadIdx.x; f < F; f += gridDim.y * DT) d[f] = src[f];
}

// dst[(b*W+w)*F + f] = src[b*F + f]   (tf.contrib.seq2seq.tile_batch), 32-bit words
__global__ __launch_bounds__(DT) void tile_rows_kernel(int W, size_t F, const uint32_t *__restrict__ src,
                                                       uint32_t *__restrict__ dst) {
  const int row = blockIdx.x, b = row / W;
  for (size_t f = (size_t)blockIdx.y * DT + threadIdx.x; f < F; f += (size_t)gridDim.y * DT)
    dst[(size_t)row * F + f] = src[(size_t)b * F + f];
}

__global__ __launch_bounds__(DT) void fill_i32_kernel(size_t n, int32_t v, int32_t *x) {
  const size_t i = (size_t)blockIdx.x * DT + threadIdx.x;
  if (i < n) x[i] = v;
}

// logprobs = [0, -inf, ...] per utterance (beam_search_decoder.py:155-157)
__global__ __launch_bounds__(DT) void beam_init_kernel(int N, int W, float *logprobs) {
  const int i = blockIdx.x * DT + threadIdx.x;
  if (i < N) logprobs[i] = (i % W) == 0 ? 0.f : -INFINITY;
}

// finalize: follow the parent pointers from the last step (one thread per final beam slot)
__global__ __launch_bounds__(DT) void beam_backtrace_kernel(int N, int W, int Tn, int Tmax,
                                                            const int32_t *__restrict__ hist_pred,
                                                            const int32_t *__restrict__ hist_parent,
                                                            int32_t *__restrict__ seq, int32_t *__restrict__ src) {
  const int row = blockIdx.x * DT + threadIdx.x;
  if (row >= N) return;
  const int b = row / W;
  int beam = row - b * W;
  for (int t = Tn - 1; t >= 0; --t) {
    const size_t o = (size_t)t * N + (size_t)b * W + beam;
    seq[(size_t)row * Tmax + t] = hist_pred[o];
    src[(size_t)row * Tmax + t] = beam;
    beam = hist_parent[o];
  }
  for (int t = Tn; t < Tmax; ++t) seq[(size_t)row * Tmax + t] = 0;
}

__global__ __launch_bounds__(DT) void beam_align_kernel(int N, int W, int Tn, int Tmax, int Te,
                                                        const float *__restrict__ hist_align,
                                                        const int32_t *__restrict__ src,
                                                        float *__restrict__ out) {
  const int row = blockIdx.x, t = blockIdx.y, b = row / W;
  float *o = out + ((size_t)row * Tmax + t) * Te;
  if (t >= Tn) {
    for (int e = threadIdx.x; e < Te; e += DT) o[e] = 0.f;
    return;
  }
  const float *a = hist_align + ((size_t)t * N + (size_t)b * W + src[(size_t)row * Tmax + t]) * Te;
  for (int e = threadIdx.x; e < Te; e += DT) o[e] = a[e];
}

__global__ __launch_bounds__(DT) void beam_scores_kernel(int N, float lpw, const float *__restrict__ logprobs,
                                                         const int32_t *__restrict__ lengths,
                                                         float *__restrict__ scores, int32_t *__restrict__ out_len) {
  const int i = blockIdx.x * DT + threadIdx.x;
  if (i >= N) return;
  scores[i] = logprobs[i] / length_penalty(lengths[i], lpw, powf(6.f, lpw));
  out_len[i] = lengths[i];
}

static int lds_fits(size_t bytes, const char *what) {
  if (bytes > 160 * 1024) return fail(NABU_EUNSUP, "%s: needs %zu bytes of LDS (160 KiB per workgroup)", what, bytes);
  return 0;
}

// ===========================================================================
// The attention beam search over M encoded inputs.  ONE loop (beam_run) for both entry points: each fills a BeamGeo and a
// BeamIO from its own descriptor and parameter struct (nabu_speller_params is the M = 1 case of the arrays).  A step is
// the cell of the Speller on B*W rows — the contexts of all mechanisms in one [N, sum E] buffer (one product, one
// gather), M alignment states — then pruning and the row gathers.  The two entry points differ in the attention step:
//   nabu_speller_beam_search        nabu_attn_fwd (with the kernels it dispatches to; its partials in the pruning scratch),
//                                   the query product against query_kernel itself;
//   nabu_speller_multi_beam_search  multi_attn_fwd, ONE launch for the step's M mechanisms (speller_multi.hip), the query
//                                   product against the column-concatenated [U, M U] kernel — also with M = 1.
constexpr int MM = NABU_SPELLER_MAX_MEMORIES;
struct BeamGeo {
  int M, B, W, U, C, nl, S, kind, K, F, prob_fn, Te[MM], E[MM], SE;
  float lpw, temperature;
  bool multi;                 // the step's attention is multi_attn_fwd
  bool sample;                // sampled decoding (W = 1): nabu_sample_advance where the search prunes and gathers
  unsigned long long seed, offset0;
  bool ctc;                   // joint CTC/attention scoring: BeamIO::ctc_logits weighted by ctcw in (0, 1)
  float ctcw;
  bool lm;                    // label n-gram fusion: BeamIO::lm_table [C^(lm_order-1), C] weighted by lmw > 0
  int lm_order;
  float lmw;
};
struct BeamIO {
  const float *values[MM];
  const int32_t *enc_len[MM];
  const float *memory_kernel[MM], *query_kernel[MM], *attention_v[MM], *conv_kernel[MM], *conv_proj[MM];
  const float *out_kernel, *out_bias, *const *lstm_kernel, *const *lstm_bias;
  float *alignments[MM];      // all null: not wanted
  int32_t *sequences, *lengths, *num_steps;
  float *scores;              // (sampled decoding: nll)
  const float *ctc_logits;    // [B, Te[0], C] logits of the CTC head on the first encoded input, or null
  const float *lm_table;      // the label n-gram's log-probabilities, or null
};

// workspace, offsets in 32-bit words
struct BeamWs {
  size_t valuesT[MM], keysB[MM], keysT[MM], lenT[MM], hist_align[MM], align[3][MM];
  size_t part[MM], wqcat, tickets;       // multi_attn_fwd only
  size_t attn_bytes;                     // nabu_attn_fwd only: its scratch, which is the pruning scratch
  size_t big, z, q, logits, acts, ids, logprobs, lengths, finished, seen, parent, stay, all_seen, scratch, hist_pred,
      hist_parent, src, gemm, gemm_bytes, total;
  size_t h[3][NABU_SPELLER_MAX_LAYERS], c[3][NABU_SPELLER_MAX_LAYERS], ctx[3];
  size_t cnorm, cstate[2], cpsi[2], clast[2], cdelta;      // joint scoring only (ctc_prefix.hip), behind everything else
  size_t lctx[2];                                          // LM fusion only: the beams' contexts, behind that
};

static BeamWs beam_ws(const BeamGeo &g) {
  BeamWs s = {};
  const size_t B = g.B, W = g.W, N = B * W, U = g.U, C = g.C, S = g.S, M = g.M, SE = g.SE;
  size_t o = 0, gb = 0;
  auto take = [&](size_t n) { size_t r = o; o += (n + 3) / 4 * 4; return r; };
  auto mx = [&](size_t v) { if (v > gb) gb = v; };
  size_t prune = B * (W * C + W);
  for (int m = 0; m < g.M; ++m) {
    const size_t Te = g.Te[m], E = g.E[m];
    s.valuesT[m] = take(N * Te * E); s.keysB[m] = take(B * Te * U); s.keysT[m] = take(N * Te * U); s.lenT[m] = take(N);
    if (g.multi) s.part[m] = take(multi_attn_part_floats((int)N, (int)Te, (int)E, (int)U, g.kind, g.K, g.F, g.prob_fn));
    s.hist_align[m] = take(S * N * Te);
    for (int k = 0; k < 3; ++k) s.align[k][m] = take(N * Te);
    mx(nabu_gemm_ws_bytes((int)(B * Te), (int)U, (int)E));
  }
  if (g.multi) {
    s.wqcat = take(U * M * U); s.tickets = take(M * N);
  } else {
    const nabu_attn_desc ad = {sizeof(nabu_attn_desc), (int32_t)N, g.Te[0], g.E[0], g.U, g.kind, g.K, g.F, g.prob_fn};
    s.attn_bytes = nabu_attn_fwd_ws_bytes(&ad);   // sliced forward (small B*W): partials
    if (s.attn_bytes / 4 > prune) prune = s.attn_bytes / 4;
  }
  s.big = take(N); s.z = take(N * 4 * U); s.q = take(N * M * U); s.logits = take(N * C);
  s.acts = take(N * 4 * U > N * M ? N * 4 * U : N * M);       // (inference: the attention's normaliser scratch, [M, N])
  s.ids = take(N); s.logprobs = take(N); s.lengths = take(N); s.finished = take(N); s.seen = take(N);
  s.parent = take(N); s.stay = take(N); s.all_seen = take(B); s.scratch = take(prune);
  s.hist_pred = take(S * N); s.hist_parent = take(S * N); s.src = take(N * S);
  for (int k = 0; k < 3; ++k) {
    for (int n = 0; n < g.nl; ++n) { s.h[k][n] = take(N * U); s.c[k][n] = take(N * U); }
    s.ctx[k] = take(N * SE);
  }
  mx(nabu_gemm_ws_bytes((int)N, (int)(4 * U), (int)SE)); mx(nabu_gemm_ws_bytes((int)N, (int)(4 * U), (int)U));
  mx(nabu_gemm_ws_bytes((int)N, (int)(M * U), (int)U)); mx(nabu_gemm_ws_bytes((int)N, (int)C, (int)U));
  mx(nabu_gemm_ws_bytes((int)N, (int)C, (int)SE));
  s.gemm_bytes = (gb + 255) / 256 * 256;
  s.gemm = take(s.gemm_bytes / 4 + 4);
  if (g.ctc) {
    const size_t T0 = g.Te[0];
    s.cnorm = take(B * T0 * 2); s.cdelta = take(N * C);
    for (int k = 0; k < 2; ++k) { s.cstate[k] = take(N * T0 * 2); s.cpsi[k] = take(N); s.clast[k] = take(N); }
  }
  if (g.lm)
    for (int k = 0; k < 2; ++k) s.lctx[k] = take(N);
  s.total = o;
  return s;
}

int ctc_prefix_lds_ok(int T);      // ctc_prefix.hip: the LDS of its kernels at T frames, NABU_EUNSUP with a message

static int check_beam(const BeamGeo &g) {
  if (g.B <= 0 || g.U <= 0 || g.C <= 1) return fail(NABU_EINVAL, "beam search: bad dimensions");
  if (g.W <= 0 || g.S <= 0) return fail(NABU_EINVAL, "beam search: beam_width and max_steps must be positive");
  if (g.sample && g.W != 1) return fail(NABU_EINVAL, "sampled decoding: beam_width must be 1");
  if (!g.sample && !(g.temperature > 0.f)) return fail(NABU_EINVAL, "beam search: temperature must be positive");
  if (g.kind < 0 || g.kind > 2 || g.prob_fn < 0 || g.prob_fn > 2)
    return fail(NABU_EINVAL, "beam search: unknown attention kind or probability_fn");
  if (g.nl < 1 || g.nl > NABU_SPELLER_MAX_LAYERS) return fail(NABU_EUNSUP, "beam search: 1..%d layers", NABU_SPELLER_MAX_LAYERS);
  if ((long long)g.B * g.W > (1 << 20)) return fail(NABU_EUNSUP, "beam search: B*beam_width too large");
  for (int m = 0; m < g.M; ++m) {
    if (g.Te[m] <= 0 || g.E[m] <= 0) return fail(NABU_EINVAL, "beam search: bad dimensions");
    if (g.U % 4 || g.E[m] % 4) return fail(NABU_EUNSUP, "beam search: num_units and encoder dim must be multiples of 4");
    const nabu_attn_desc a = {sizeof(nabu_attn_desc), g.B * g.W, g.Te[m], g.E[m], g.U, g.kind, g.K, g.F, g.prob_fn};
    if (g.multi && nabu_attn_bwd_slices(&a) <= 0) return NABU_EUNSUP;       // (its kernels' LDS: the message is theirs)
  }
  return 0;
}

// The optional CTC operand of the *_joint entry points: absent (null) or weight 0 leaves g as it is — the loop then makes
// exactly the launches of the plain search; otherwise g.ctc is set.
static int beam_ctc(BeamGeo *g, const float *ctc_logits, float ctc_weight) {
  if (!(ctc_weight >= 0.f && ctc_weight < 1.f)) return fail(NABU_EINVAL, "beam search: ctc_weight must be in [0, 1)");
  if (!ctc_logits || ctc_weight == 0.f) return 0;
  g->ctc = true; g->ctcw = ctc_weight;
  return ctc_prefix_lds_ok(g->Te[0]);
}

// The dense label n-gram of the *_lm / *_ex entry points: [C^(order-1), C] log-probabilities, C^order entries, at most
// 2^24 of them (64 MiB).  *nctx = C^(order-1).
constexpr long long LM_MAX_ENTRIES = 1ll << 24;
static int lm_contexts(const char *what, int C, int order, int *nctx) {
  if (order < 1) return fail(NABU_EINVAL, "%s: lm_order must be at least 1, got %d", what, order);
  long long n = 1;
  for (int k = 0; k < order; ++k) {
    n *= C;
    if (n > LM_MAX_ENTRIES)
      return fail(NABU_EUNSUP, "%s: a table of %d^%d entries exceeds the limit of 2^24 entries (64 MiB)", what, C, order);
  }
  *nctx = (int)(n / C);
  return 0;
}

// The optional LM operand of the *_ex entry points: absent (null) or weight 0 leaves g as it is — the loop then makes
// exactly the launches it makes without one; otherwise g.lm is set.
static int beam_lm(BeamGeo *g, const float *lm_table, int lm_order, float lm_weight) {
  if (!(lm_weight >= 0.f && lm_weight <= FLT_MAX)) return fail(NABU_EINVAL, "beam search: lm_weight must be finite and >= 0");
  if (!lm_table || lm_weight == 0.f) return 0;
  int nctx;
  if (int e = lm_contexts("beam search", g->C, lm_order, &nctx)) return e;
  g->lm = true; g->lm_order = lm_order; g->lmw = lm_weight;
  return 0;
}

static int beam_run(const BeamGeo &g, const BeamIO &io, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(io.out_kernel && io.out_bias && io.sequences && io.lengths && io.scores && io.num_steps && ws,
                 "beam search: null pointer");
  for (int m = 0; m < g.M; ++m)
    NABU_CHECK_ARG(io.values[m] && io.enc_len[m] && io.memory_kernel[m] && io.query_kernel[m] && io.attention_v[m] &&
                   (g.kind != 1 || (io.conv_kernel[m] && io.conv_proj[m])) && (!io.alignments[0] || io.alignments[m]),
                   "beam search: null pointer for an encoded input");
  NABU_CHECK_ARG(!g.ctc || io.ctc_logits, "beam search: null pointer for the CTC logits");
  NABU_CHECK_ARG(!g.lm || (io.lm_table && !g.sample), "beam search: null pointer for the LM table");
  const BeamWs L = beam_ws(g);
  if (ws_bytes < L.total * 4) return fail(NABU_EWS, "beam search: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float *w = static_cast<float *>(ws);
  int32_t *wi = static_cast<int32_t *>(ws);
  const int B = g.B, W = g.W, N = B * W, U = g.U, C = g.C, nl = g.nl, S = g.S, M = g.M, SE = g.SE, MU = M * U;
  float *gw = w + L.gemm;
  const size_t gwb = L.gemm_bytes;
  const nabu_attn_desc ad = {sizeof(nabu_attn_desc), N, g.Te[0], g.E[0], U, g.kind, g.K, g.F, g.prob_fn};
  auto tile = [&](const void *src, void *dst, size_t F) {
    size_t gy = (F + DT * 4 - 1) / (DT * 4);
    hipLaunchKernelGGL(tile_rows_kernel, dim3(N, gy > 64 ? 64 : (unsigned)gy), dim3(DT), 0, s, W, F,
                       static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst));
  };
  // tile_batch of the encoder outputs / their lengths; keys = memory_layer(values) once per utterance
  for (int m = 0; m < M; ++m) {
    const int Te = g.Te[m], E = g.E[m];
    NABU_TRY(mm(0, 0, B * Te, U, E, io.values[m], E, io.memory_kernel[m], U, 0.f, w + L.keysB[m], U, nullptr, gw, gwb, stream));
    tile(io.values[m], w + L.valuesT[m], (size_t)Te * E);
    tile(w + L.keysB[m], w + L.keysT[m], (size_t)Te * U);
    tile(io.enc_len[m], wi + L.lenT[m], 1);
    NABU_LAUNCH_CHECK();
    if (g.multi) NABU_TRY(put_cols(U, U, io.query_kernel[m], w + L.wqcat, MU, m * U, s));
  }
  const float *wq = g.multi ? w + L.wqcat : io.query_kernel[0];     // [U, M U]
  const int gN = (N + DT - 1) / DT;
  hipLaunchKernelGGL(fill_i32_kernel, dim3(gN), dim3(DT), 0, s, (size_t)N, INT_MAX, wi + L.big);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(gN), dim3(DT), 0, s, (size_t)N, C - 1, wi + L.ids);       // start tokens
  hipLaunchKernelGGL(beam_init_kernel, dim3(gN), dim3(DT), 0, s, N, W, w + L.logprobs);
  NABU_LAUNCH_CHECK();
  NABU_HIP(hipMemsetAsync(wi + L.lengths, 0, (size_t)N * 4, s));
  NABU_HIP(hipMemsetAsync(wi + L.finished, 0, (size_t)N * 4, s));
  NABU_HIP(hipMemsetAsync(wi + L.seen, 0, (size_t)N * 4, s));
  if (g.multi) NABU_HIP(hipMemsetAsync(wi + L.tickets, 0, (size_t)M * N * 4, s));
  if (g.sample) {                                  // written in place by every step: sequences [B,S], lengths, nll [B]
    NABU_HIP(hipMemsetAsync(io.sequences, 0, (size_t)N * S * 4, s));
    NABU_HIP(hipMemsetAsync(io.lengths, 0, (size_t)N * 4, s));
    NABU_HIP(hipMemsetAsync(io.scores, 0, (size_t)N * 4, s));
    NABU_HIP(hipMemsetAsync(wi + L.src, 0, (size_t)N * S * 4, s));       // (beam_align_kernel: slot 0 at every step)
  }
  int cur = 0, fresh = 1, nxt = 2;                 // state sets: before the step, after the cell, after pruning
  for (int n = 0; n < nl; ++n) {
    NABU_HIP(hipMemsetAsync(w + L.h[cur][n], 0, (size_t)N * U * 4, s));
    NABU_HIP(hipMemsetAsync(w + L.c[cur][n], 0, (size_t)N * U * 4, s));
  }
  NABU_HIP(hipMemsetAsync(w + L.ctx[cur], 0, (size_t)N * SE * 4, s));
  for (int m = 0; m < M; ++m) {
    NABU_HIP(hipMemsetAsync(w + L.align[cur][m], 0, (size_t)N * g.Te[m] * 4, s));
    if (g.kind == 2) NABU_TRY(first_col_one(N, g.Te[m], w + L.align[cur][m], s));
  }
  // joint scoring: the CTC prefix state of the empty hypothesis in every slot; set cc is the current one
  int cc = 0;
  const int T0 = g.Te[0];
  if (g.ctc)
    NABU_TRY(nabu_ctc_prefix_prepare(B, W, T0, C, io.ctc_logits, io.enc_len[0], w + L.cnorm, w + L.cstate[0], w + L.cpsi[0],
                                     wi + L.clast[0], stream));
  // LM fusion: the context of the empty hypothesis (every digit the boundary C-1) in every slot; set lc is the current one
  int lc = 0, nctx = 1;
  if (g.lm) {
    NABU_TRY(lm_contexts("beam search", C, g.lm_order, &nctx));
    hipLaunchKernelGGL(fill_i32_kernel, dim3(gN), dim3(DT), 0, s, (size_t)N, nctx - 1, wi + L.lctx[0]);
    NABU_LAUNCH_CHECK();
  }
  float *z = w + L.z, *lg = w + L.logits;
  const int32_t *big = wi + L.big;
  int32_t *par = wi + L.parent, *stay = wi + L.stay;
  const int ndone = g.sample ? 1 : B;              // flags of the stop test: all_finished[0], or all_seen [B]
  std::vector<int32_t> done(ndone);
  int Tn = 0;
  for (int t = 0; t < S; ++t) {
    // the cell on all B*W rows (the step of nabu_speller_fwd / nabu_speller_multi_fwd; no dropout at inference)
    for (int n = 0; n < nl; ++n) {
      const float *Kn = io.lstm_kernel[n];
      if (n == 0) {
        NABU_TRY(mm(0, 0, N, 4 * U, SE, w + L.ctx[cur], SE, Kn + (size_t)C * 4 * U, 4 * U, 0.f, z, 4 * U, nullptr, gw, gwb, stream));
        NABU_TRY(mm(0, 0, N, 4 * U, U, w + L.h[cur][0], U, Kn + (size_t)(C + SE) * 4 * U, 4 * U, 1.f, z, 4 * U, nullptr, gw, gwb, stream));
        NABU_TRY(nabu_lstm_cell_fwd(N, U, 0, big, z, io.lstm_bias[0], Kn, wi + L.ids, w + L.c[cur][0], w + L.h[cur][0],
                                    w + L.acts, w + L.c[fresh][0], w + L.h[fresh][0], stream));
      } else {
        NABU_TRY(mm(0, 0, N, 4 * U, U, w + L.h[fresh][n - 1], U, Kn, 4 * U, 0.f, z, 4 * U, nullptr, gw, gwb, stream));
        NABU_TRY(mm(0, 0, N, 4 * U, U, w + L.h[cur][n], U, Kn + (size_t)U * 4 * U, 4 * U, 1.f, z, 4 * U, nullptr, gw, gwb, stream));
        NABU_TRY(nabu_lstm_cell_fwd(N, U, 0, big, z, io.lstm_bias[n], nullptr, nullptr, w + L.c[cur][n], w + L.h[cur][n],
                                    w + L.acts, w + L.c[fresh][n], w + L.h[fresh][n], stream));
      }
    }
    const float *htop = w + L.h[fresh][nl - 1];
    NABU_TRY(mm(0, 0, N, MU, U, htop, U, wq, MU, 0.f, w + L.q, MU, nullptr, gw, gwb, stream));
    // (normaliser scratch of the attention: w + L.acts — the saved gate activations are not used at inference)
    if (g.multi) {
      MultiAttnMem mem[MM];
      for (int m = 0; m < M; ++m)
        mem[m] = MultiAttnMem{g.Te[m], g.E[m], wi + L.lenT[m], w + L.keysT[m], w + L.valuesT[m], io.attention_v[m],
                              io.conv_kernel[m], io.conv_proj[m], w + L.align[cur][m], w + L.align[fresh][m],
                              w + L.acts + (size_t)m * N, w + L.part[m],
                              reinterpret_cast<unsigned *>(wi + L.tickets) + (size_t)m * N};
      NABU_TRY(multi_attn_fwd(M, N, U, g.kind, g.K, g.F, g.prob_fn, 0, big, w + L.q, w + L.ctx[cur], w + L.ctx[fresh], mem, s));
    } else {
      NABU_TRY(nabu_attn_fwd(&ad, 0, big, wi + L.lenT[0], w + L.keysT[0], w + L.valuesT[0], w + L.q, io.attention_v[0],
                             io.conv_kernel[0], io.conv_proj[0], w + L.align[cur][0], w + L.ctx[cur], w + L.align[fresh][0],
                             w + L.ctx[fresh], w + L.acts, w + L.scratch, L.attn_bytes, stream));
    }
    // AttentionProjectionWrapper: [h, contexts of this step]·W + b (rnn_cell.py:145-155)
    NABU_TRY(mm(0, 0, N, C, U, htop, U, io.out_kernel, C, 0.f, lg, C, io.out_bias, gw, gwb, stream));
    NABU_TRY(mm(0, 0, N, C, SE, w + L.ctx[fresh], SE, io.out_kernel + (size_t)U * C, C, 1.f, lg, C, nullptr, gw, gwb, stream));
    const int adv = g.sample ? fresh : nxt;        // the state set the next step starts from
    if (g.sample) {
      // draw the next input of every row; no parent and no stay: the cell's fresh state is the next step's
      NABU_TRY(nabu_sample_advance(B, C, lg, g.seed, g.offset0 + (unsigned long long)t, t, S, io.sequences, io.lengths,
                                   wi + L.finished, io.scores, wi + L.ids, wi + L.all_seen, stream));
    } else {
      // expand + prune; the predicted ids are the next step's inputs
      if (g.lm) {
        // the LM term is looked up inside the prune (no launch of its own), which also writes the survivors' contexts
        if (g.ctc)
          NABU_TRY(nabu_ctc_prefix_score(B, W, T0, C, io.ctc_logits, io.enc_len[0], w + L.cnorm, w + L.cstate[cc], w + L.cpsi[cc],
                                         wi + L.clast[cc], wi + L.finished, w + L.cdelta, stream));
        NABU_TRY(nabu_beam_prune_lm(B, W, C, lg, g.ctc ? w + L.cdelta : nullptr, g.ctc ? g.ctcw : 0.f, io.lm_table, g.lm_order,
                                    g.lmw, wi + L.lctx[lc], wi + L.lctx[lc ^ 1], g.temperature, g.lpw, w + L.logprobs,
                                    wi + L.lengths, wi + L.finished, wi + L.seen, wi + L.ids, par, stay, wi + L.all_seen,
                                    w + L.scratch, stream));
        lc ^= 1;
        if (g.ctc) {
          NABU_TRY(nabu_ctc_prefix_advance(B, W, T0, C, io.ctc_logits, io.enc_len[0], w + L.cnorm, w + L.cstate[cc],
                                           w + L.cpsi[cc], wi + L.clast[cc], par, stay, wi + L.ids, w + L.cstate[cc ^ 1],
                                           w + L.cpsi[cc ^ 1], wi + L.clast[cc ^ 1], stream));
          cc ^= 1;
        }
      } else if (g.ctc) {
        // the CTC prefix score of every (hypothesis, label), mixed into the candidates; then the survivors' states
        NABU_TRY(nabu_ctc_prefix_score(B, W, T0, C, io.ctc_logits, io.enc_len[0], w + L.cnorm, w + L.cstate[cc], w + L.cpsi[cc],
                                       wi + L.clast[cc], wi + L.finished, w + L.cdelta, stream));
        NABU_TRY(nabu_beam_prune_joint(B, W, C, lg, w + L.cdelta, g.ctcw, g.temperature, g.lpw, w + L.logprobs,
                                       wi + L.lengths, wi + L.finished, wi + L.seen, wi + L.ids, par, stay,
                                       wi + L.all_seen, w + L.scratch, stream));
        NABU_TRY(nabu_ctc_prefix_advance(B, W, T0, C, io.ctc_logits, io.enc_len[0], w + L.cnorm, w + L.cstate[cc],
                                         w + L.cpsi[cc], wi + L.clast[cc], par, stay, wi + L.ids, w + L.cstate[cc ^ 1],
                                         w + L.cpsi[cc ^ 1], wi + L.clast[cc ^ 1], stream));
        cc ^= 1;
      } else {
        NABU_TRY(nabu_beam_prune(B, W, C, lg, g.temperature, g.lpw, w + L.logprobs, wi + L.lengths, wi + L.finished,
                                 wi + L.seen, wi + L.ids, par, stay, wi + L.all_seen, w + L.scratch, stream));
      }
      for (int n = 0; n < nl; ++n) {
        NABU_TRY(nabu_beam_gather(B, W, U, w + L.h[fresh][n], w + L.h[cur][n], par, stay, w + L.h[nxt][n], stream));
        NABU_TRY(nabu_beam_gather(B, W, U, w + L.c[fresh][n], w + L.c[cur][n], par, stay, w + L.c[nxt][n], stream));
      }
      NABU_TRY(nabu_beam_gather(B, W, SE, w + L.ctx[fresh], w + L.ctx[cur], par, stay, w + L.ctx[nxt], stream));
      for (int m = 0; m < M; ++m)
        NABU_TRY(nabu_beam_gather(B, W, g.Te[m], w + L.align[fresh][m], w + L.align[cur][m], par, stay, w + L.align[nxt][m], stream));
      NABU_HIP(hipMemcpyAsync(wi + L.hist_pred + (size_t)t * N, wi + L.ids, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
      NABU_HIP(hipMemcpyAsync(wi + L.hist_parent + (size_t)t * N, par, (size_t)N * 4, hipMemcpyDeviceToDevice, s));
    }
    for (int m = 0; m < M; ++m)
      NABU_HIP(hipMemcpyAsync(w + L.hist_align[m] + (size_t)t * N * g.Te[m], w + L.align[adv][m], (size_t)N * g.Te[m] * 4,
                              hipMemcpyDeviceToDevice, s));
    int &old = g.sample ? fresh : nxt;             // cur and the advanced set change places
    const int tmp = cur; cur = adv; old = tmp;
    Tn = t + 1;
    // dynamic_decode's stop test: every slot has been finished at some step
    NABU_HIP(hipMemcpyAsync(done.data(), wi + L.all_seen, (size_t)ndone * 4, hipMemcpyDeviceToHost, s));
    NABU_HIP(hipStreamSynchronize(s));
    bool all = true;
    for (int b = 0; b < ndone; ++b) all = all && done[b] != 0;
    if (all) break;
  }
  // finalize (beam_search_decoder.py:341-451); a sampled decode has its sequences, lengths and nll already
  if (!g.sample) {
    hipLaunchKernelGGL(beam_backtrace_kernel, dim3(gN), dim3(DT), 0, s, N, W, Tn, S, wi + L.hist_pred, wi + L.hist_parent,
                       io.sequences, wi + L.src);
    NABU_LAUNCH_CHECK();
  }
  for (int m = 0; m < M && io.alignments[0]; ++m) {
    hipLaunchKernelGGL(beam_align_kernel, dim3(N, S), dim3(DT), 0, s, N, W, Tn, S, g.Te[m], w + L.hist_align[m], wi + L.src,
                       io.alignments[m]);
    NABU_LAUNCH_CHECK();
  }
  if (!g.sample) {
    hipLaunchKernelGGL(beam_scores_kernel, dim3(gN), dim3(DT), 0, s, N, g.lpw, w + L.logprobs, wi + L.lengths, io.scores,
                       io.lengths);
    NABU_LAUNCH_CHECK();
  }
  *io.num_steps = Tn;
  return 0;
}

// the two descriptors as a BeamGeo (checked)
static int beam_geo(const nabu_beam_desc *d, BeamGeo *g, bool sample = false) {
  if (!d || d->size != sizeof(nabu_beam_desc)) return fail(NABU_EINVAL, "beam search: bad descriptor size");
  *g = BeamGeo{1, d->B, d->beam_width, d->U, d->C, d->num_layers, d->max_steps, d->kind, d->K, d->F, d->prob_fn,
               {d->Te}, {d->E}, d->E, d->length_penalty, d->temperature, false, sample};
  return check_beam(*g);
}
static int beam_geo(const nabu_multi_beam_desc *d, BeamGeo *g, bool sample = false) {
  if (!d || d->size != sizeof(nabu_multi_beam_desc)) return fail(NABU_EINVAL, "multi beam search: bad descriptor size");
  if (d->M < 1 || d->M > MM) return fail(NABU_EUNSUP, "multi beam search: 1..%d encoded inputs", MM);
  *g = BeamGeo{d->M, d->B, d->beam_width, d->U, d->C, d->num_layers, d->max_steps, d->kind, d->K, d->F, d->prob_fn,
               {}, {}, 0, d->length_penalty, d->temperature, true, sample};
  for (int m = 0; m < d->M; ++m) { g->Te[m] = d->Te[m]; g->E[m] = d->E[m]; g->SE += d->E[m]; }
  return check_beam(*g);
}

}  // namespace nabu

using namespace nabu;

extern "C" size_t nabu_ctc_beam_ws_bytes(int B, int T, int C, int beam_width) {
  if (B <= 0 || T <= 0 || C <= 1 || beam_width <= 0) return 0;
  const size_t NN = 1 + (size_t)T * beam_width;
  return (size_t)B * NN * (3 + (size_t)C - 1) * 4;
}

// the prefix trees with the two words a node keeps for the LM (context, the term it entered with)
extern "C" size_t nabu_ctc_beam_lm_ws_bytes(int B, int T, int C, int beam_width) {
  if (B <= 0 || T <= 0 || C <= 1 || beam_width <= 0) return 0;
  const size_t NN = 1 + (size_t)T * beam_width;
  return (size_t)B * NN * (5 + (size_t)C - 1) * 4;
}

// both searches: lm_table null is the plain one
static int ctc_beam(const char *what, int B, int T, int C, int beam_width, int merge_repeated, const float *logits,
                    const int32_t *logit_len, const float *lm_table, int nctx, float alpha, float beta, int32_t *out_ids,
                    int32_t *out_len, float *out_logprob, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  if (B <= 0 || T <= 0 || C <= 1 || beam_width <= 0) return fail(NABU_EINVAL, "%s: bad dimensions", what);
  if (!(logits && logit_len && out_ids && out_len && ws)) return fail(NABU_EINVAL, "%s: null pointer", what);
  if (beam_width > DT) return fail(NABU_EUNSUP, "%s: beam_width <= %d", what, DT);
  const size_t need = lm_table ? nabu_ctc_beam_lm_ws_bytes(B, T, C, beam_width) : nabu_ctc_beam_ws_bytes(B, T, C, beam_width);
  if (ws_bytes < need) return fail(NABU_EWS, "%s: workspace too small", what);
  const size_t lds = ctc_beam_lds(C, beam_width);
  NABU_TRY(lds_fits(lds, what));
  hipStream_t s = static_cast<hipStream_t>(stream);
  NABU_HIP(hipMemsetAsync(ws, 0xFF, need, s));   // every tree pointer = -1
  CtcBeamLmArgs a;
  a.B = B; a.T = T; a.C = C; a.W = beam_width; a.merge = merge_repeated ? 1 : 0;
  a.NN = 1 + T * beam_width;
  a.logits = logits; a.len = logit_len; a.out_ids = out_ids; a.out_len = out_len; a.out_lp = out_logprob;
  a.nodes = static_cast<int32_t *>(ws);
  a.per_utt = (size_t)a.NN * ((lm_table ? 5 : 3) + (size_t)C - 1);
  a.lm = lm_table; a.nctx = nctx; a.alpha = alpha; a.beta = beta;
  if (lm_table) return launch_lds(ctc_beam_kernel<true>, dim3(B), dim3(DT), lds, s, a);
  return launch_lds(ctc_beam_kernel<false>, dim3(B), dim3(DT), lds, s, static_cast<const CtcBeamArgs &>(a));
}

extern "C" int nabu_ctc_beam_search(int B, int T, int C, int beam_width, int merge_repeated, const float *logits,
                                    const int32_t *logit_len, int32_t *out_ids, int32_t *out_len,
                                    float *out_logprob, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  return ctc_beam("ctc_beam_search", B, T, C, beam_width, merge_repeated, logits, logit_len, nullptr, 1, 0.f, 0.f, out_ids,
                  out_len, out_logprob, ws, ws_bytes, stream);
}

extern "C" int nabu_ctc_beam_search_lm(int B, int T, int C, int beam_width, int merge_repeated, const float *logits,
                                       const int32_t *logit_len, const float *lm_table, int lm_order, float lm_weight,
                                       float insertion_bonus, int32_t *out_ids, int32_t *out_len, float *out_logprob,
                                       void *ws, size_t ws_bytes, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && T > 0 && C > 1 && beam_width > 0, "ctc_beam_search_lm: bad dimensions");
  NABU_CHECK_ARG(lm_table, "ctc_beam_search_lm: null pointer");
  NABU_CHECK_ARG(lm_weight >= 0.f && lm_weight <= FLT_MAX, "ctc_beam_search_lm: lm_weight must be finite and >= 0");
  NABU_CHECK_ARG(insertion_bonus >= -FLT_MAX && insertion_bonus <= FLT_MAX, "ctc_beam_search_lm: insertion_bonus must be finite");
  int nctx;
  if (int e = lm_contexts("ctc_beam_search_lm", C, lm_order, &nctx)) return e;
  return ctc_beam("ctc_beam_search_lm", B, T, C, beam_width, merge_repeated, logits, logit_len, lm_table, nctx, lm_weight,
                  insertion_bonus, out_ids, out_len, out_logprob, ws, ws_bytes, stream);
}

extern "C" int nabu_edit_distance(int B, const int32_t *hyp, int ldh, const int32_t *hyp_len, const int32_t *truth,
                                  int ldt, const int32_t *truth_len, int32_t *dist, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && ldh >= 0 && ldt >= 0, "edit_distance: bad dimensions");
  NABU_CHECK_ARG(hyp_len && truth_len && dist && (hyp || ldh == 0) && (truth || ldt == 0), "edit_distance: null pointer");
  const size_t lds = 3 * ((size_t)ldh + 1) * 4;
  NABU_TRY(lds_fits(lds, "edit_distance"));
  return launch_lds(edit_distance_kernel, dim3(B), dim3(DT), lds, static_cast<hipStream_t>(stream), B, hyp, ldh, hyp_len,
                    truth, ldt, truth_len, dist);
}

extern "C" int nabu_beam_prune(int B, int W, int C, const float *logits, float temperature, float length_penalty_w,
                               float *logprobs, int32_t *lengths, int32_t *finished, int32_t *seen,
                               int32_t *pred_ids, int32_t *parent, int32_t *stay, int32_t *all_seen,
                               float *scratch, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && W > 0 && C > 1 && temperature > 0.f, "beam_prune: bad arguments");
  NABU_CHECK_ARG(logits && logprobs && lengths && finished && seen && pred_ids && parent && stay && all_seen && scratch,
                 "beam_prune: null pointer");
  const size_t lds = 5 * (size_t)W * 4;
  NABU_TRY(lds_fits(lds, "beam_prune"));
  PruneArgs a = {B, W, C, logits, 1.f / temperature, length_penalty_w, logprobs, lengths, finished, seen,
                 pred_ids, parent, stay, all_seen, scratch, nullptr, 0.f};
  return launch_lds(beam_prune_kernel<false, false>, dim3(B), dim3(DT), lds, static_cast<hipStream_t>(stream), a);
}

extern "C" int nabu_beam_prune_joint(int B, int W, int C, const float *logits, const float *delta, float ctc_weight,
                                     float temperature, float length_penalty_w, float *logprobs, int32_t *lengths,
                                     int32_t *finished, int32_t *seen, int32_t *pred_ids, int32_t *parent,
                                     int32_t *stay, int32_t *all_seen, float *scratch, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && W > 0 && C > 1 && temperature > 0.f, "beam_prune_joint: bad arguments");
  NABU_CHECK_ARG(ctc_weight >= 0.f && ctc_weight < 1.f, "beam_prune_joint: ctc_weight must be in [0, 1)");   // (false for NaN)
  NABU_CHECK_ARG(logits && delta && logprobs && lengths && finished && seen && pred_ids && parent && stay && all_seen &&
                 scratch, "beam_prune_joint: null pointer");
  const size_t lds = 5 * (size_t)W * 4;
  NABU_TRY(lds_fits(lds, "beam_prune_joint"));
  PruneArgs a = {B, W, C, logits, 1.f / temperature, length_penalty_w, logprobs, lengths, finished, seen,
                 pred_ids, parent, stay, all_seen, scratch, delta, ctc_weight};
  return launch_lds(beam_prune_kernel<true, false>, dim3(B), dim3(DT), lds, static_cast<hipStream_t>(stream), a);
}

extern "C" int nabu_beam_prune_lm(int B, int W, int C, const float *logits, const float *delta, float ctc_weight,
                                  const float *lm_table, int lm_order, float lm_weight, const int32_t *ctx_in,
                                  int32_t *ctx_out, float temperature, float length_penalty_w, float *logprobs,
                                  int32_t *lengths, int32_t *finished, int32_t *seen, int32_t *pred_ids, int32_t *parent,
                                  int32_t *stay, int32_t *all_seen, float *scratch, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && W > 0 && C > 1 && temperature > 0.f, "beam_prune_lm: bad arguments");
  NABU_CHECK_ARG(ctc_weight >= 0.f && ctc_weight < 1.f, "beam_prune_lm: ctc_weight must be in [0, 1)");      // (false for NaN)
  NABU_CHECK_ARG(lm_weight >= 0.f && lm_weight <= FLT_MAX, "beam_prune_lm: lm_weight must be finite and >= 0");
  NABU_CHECK_ARG(logits && lm_table && ctx_in && ctx_out && ctx_in != ctx_out && logprobs && lengths && finished && seen &&
                 pred_ids && parent && stay && all_seen && scratch, "beam_prune_lm: null pointer");
  int nctx;
  if (int e = lm_contexts("beam_prune_lm", C, lm_order, &nctx)) return e;
  const size_t lds = 6 * (size_t)W * 4;
  NABU_TRY(lds_fits(lds, "beam_prune_lm"));
  PruneLmArgs a;
  static_cast<PruneArgs &>(a) = PruneArgs{B, W, C, logits, 1.f / temperature, length_penalty_w, logprobs, lengths, finished,
                                          seen, pred_ids, parent, stay, all_seen, scratch, delta, delta ? ctc_weight : 0.f};
  a.lm = lm_table; a.nctx = nctx; a.lmw = lm_weight; a.ctx_in = ctx_in; a.ctx_out = ctx_out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (delta) return launch_lds(beam_prune_kernel<true, true>, dim3(B), dim3(DT), lds, s, a);
  return launch_lds(beam_prune_kernel<false, true>, dim3(B), dim3(DT), lds, s, a);
}

extern "C" int nabu_beam_gather(int B, int W, int F, const float *fresh, const float *old, const int32_t *parent,
                                const int32_t *stay, float *dst, nabu_stream_t stream) {
  NABU_CHECK_ARG(B > 0 && W > 0 && F > 0, "beam_gather: bad dimensions");
  NABU_CHECK_ARG(fresh && old && parent && stay && dst, "beam_gather: null pointer");
  const int gy = (F + DT * 4 - 1) / (DT * 4);
  hipLaunchKernelGGL(beam_gather_kernel, dim3(B * W, gy > 64 ? 64 : gy), dim3(DT), 0,
                     static_cast<hipStream_t>(stream), W, F, fresh, old, parent, stay, dst);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" int nabu_sample_advance(int B, int C, const float *logits, unsigned long long seed, unsigned long long offset,
                                   int t, int max_steps, int32_t *sequences, int32_t *lengths, int32_t *finished,
                                   float *nll, int32_t *next_ids, int32_t *all_finished, nabu_stream_t stream) {
  if (B == 0) return 0;
  NABU_CHECK_ARG(B > 0 && C > 0 && t >= 0 && t < max_steps, "sample_advance: bad arguments");
  NABU_CHECK_ARG(logits && sequences && lengths && finished && nll && next_ids && all_finished,
                 "sample_advance: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(DT), 0, s, (size_t)1, 1, all_finished);
  const SampleArgs a = {C, t, max_steps, logits, seed, offset, sequences, lengths, finished, next_ids, all_finished, nll};
  hipLaunchKernelGGL(sample_advance_kernel, dim3(B), dim3(64), C <= SAMPLE_LDS_C ? (size_t)C * 4 : 0, s, a);
  NABU_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t nabu_speller_beam_ws_bytes(const nabu_beam_desc *d) {
  BeamGeo g;
  return beam_geo(d, &g) ? 0 : beam_ws(g).total * 4;
}

// the search (sample = false: scores) or the sampled decode (nll) of one encoded input
static int decode_one(BeamGeo &g, const float *values, const int32_t *enc_len, const nabu_speller_params *p,
                      int32_t *sequences, int32_t *lengths, float *scores, float *alignments, int32_t *num_steps, void *ws,
                      size_t ws_bytes, nabu_stream_t stream, const float *ctc_logits = nullptr,
                      const float *lm_table = nullptr) {
  NABU_CHECK_ARG(p, "speller_beam_search: null pointer");
  const BeamIO io = {{values}, {enc_len}, {p->memory_kernel}, {p->query_kernel}, {p->attention_v}, {p->conv_kernel},
                     {p->conv_proj}, p->out_kernel, p->out_bias, p->lstm_kernel, p->lstm_bias, {alignments},
                     sequences, lengths, num_steps, scores, ctc_logits, lm_table};
  return beam_run(g, io, ws, ws_bytes, stream);
}

extern "C" int nabu_speller_beam_search(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                        const nabu_speller_params *p, int32_t *sequences, int32_t *lengths,
                                        float *scores, float *alignments, int32_t *num_steps, void *ws,
                                        size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  return decode_one(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream);
}

extern "C" size_t nabu_speller_beam_joint_ws_bytes(const nabu_beam_desc *d) {
  BeamGeo g;
  if (beam_geo(d, &g)) return 0;
  g.ctc = true;
  return ctc_prefix_lds_ok(g.Te[0]) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_beam_search_joint(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                              const nabu_speller_params *p, const float *ctc_logits, float ctc_weight,
                                              int32_t *sequences, int32_t *lengths, float *scores, float *alignments,
                                              int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  if (int e = beam_ctc(&g, ctc_logits, ctc_weight)) return e;
  return decode_one(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream,
                    ctc_logits);
}

// the options of the *_ex entry points as flags of the geometry (checked)
static int beam_opts(BeamGeo *g, const nabu_beam_search_opts *o) {
  if (!o || o->size != sizeof(nabu_beam_search_opts)) return fail(NABU_EINVAL, "beam search: bad options size");
  if (int e = beam_ctc(g, o->ctc_logits, o->ctc_weight)) return e;
  return beam_lm(g, o->lm_table, o->lm_order, o->lm_weight);
}

extern "C" size_t nabu_speller_beam_ex_ws_bytes(const nabu_beam_desc *d, const nabu_beam_search_opts *o) {
  BeamGeo g;
  return beam_geo(d, &g) || beam_opts(&g, o) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_beam_search_ex(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                           const nabu_speller_params *p, const nabu_beam_search_opts *o,
                                           int32_t *sequences, int32_t *lengths, float *scores, float *alignments,
                                           int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  if (int e = beam_opts(&g, o)) return e;
  return decode_one(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream,
                    o->ctc_logits, o->lm_table);
}

extern "C" size_t nabu_speller_sample_ws_bytes(const nabu_beam_desc *d) {
  BeamGeo g;
  return beam_geo(d, &g, true) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_sample(const nabu_beam_desc *d, const float *values, const int32_t *enc_len,
                                   const nabu_speller_params *p, unsigned long long seed, unsigned long long offset0,
                                   int32_t *sequences, int32_t *lengths, float *nll, float *alignments,
                                   int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g, true)) return e;
  g.seed = seed; g.offset0 = offset0;
  return decode_one(g, values, enc_len, p, sequences, lengths, nll, alignments, num_steps, ws, ws_bytes, stream);
}

extern "C" size_t nabu_speller_multi_beam_ws_bytes(const nabu_multi_beam_desc *d) {
  BeamGeo g;
  return beam_geo(d, &g) ? 0 : beam_ws(g).total * 4;
}

// the same over M encoded inputs
static int decode_multi(BeamGeo &g, const float *const *values, const int32_t *const *enc_len,
                        const nabu_speller_multi_params *p, int32_t *sequences, int32_t *lengths, float *scores,
                        float *const *alignments, int32_t *num_steps, void *ws, size_t ws_bytes, nabu_stream_t stream,
                        const float *ctc_logits = nullptr, const float *lm_table = nullptr) {
  NABU_CHECK_ARG(values && enc_len && p, "speller_multi_beam_search: null pointer");
  BeamIO io = {{}, {}, {}, {}, {}, {}, {}, p->out_kernel, p->out_bias, p->lstm_kernel, p->lstm_bias, {},
               sequences, lengths, num_steps, scores, ctc_logits, lm_table};
  for (int m = 0; m < g.M; ++m) {
    io.values[m] = values[m]; io.enc_len[m] = enc_len[m];
    io.memory_kernel[m] = p->memory_kernel[m]; io.query_kernel[m] = p->query_kernel[m];
    io.attention_v[m] = p->attention_v[m]; io.conv_kernel[m] = p->conv_kernel[m]; io.conv_proj[m] = p->conv_proj[m];
    if (alignments) {
      NABU_CHECK_ARG(alignments[m], "speller_multi_beam_search: null pointer for an encoded input");
      io.alignments[m] = alignments[m];
    }
  }
  return beam_run(g, io, ws, ws_bytes, stream);
}

extern "C" int nabu_speller_multi_beam_search(const nabu_multi_beam_desc *d, const float *const *values,
                                              const int32_t *const *enc_len, const nabu_speller_multi_params *p,
                                              int32_t *sequences, int32_t *lengths, float *scores,
                                              float *const *alignments, int32_t *num_steps, void *ws, size_t ws_bytes,
                                              nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  return decode_multi(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream);
}

extern "C" size_t nabu_speller_multi_beam_joint_ws_bytes(const nabu_multi_beam_desc *d) {
  BeamGeo g;
  if (beam_geo(d, &g)) return 0;
  g.ctc = true;
  return ctc_prefix_lds_ok(g.Te[0]) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_multi_beam_search_joint(const nabu_multi_beam_desc *d, const float *const *values,
                                                    const int32_t *const *enc_len, const nabu_speller_multi_params *p,
                                                    const float *ctc_logits, float ctc_weight, int32_t *sequences,
                                                    int32_t *lengths, float *scores, float *const *alignments,
                                                    int32_t *num_steps, void *ws, size_t ws_bytes,
                                                    nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  if (int e = beam_ctc(&g, ctc_logits, ctc_weight)) return e;
  return decode_multi(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream,
                      ctc_logits);
}

extern "C" size_t nabu_speller_multi_beam_ex_ws_bytes(const nabu_multi_beam_desc *d, const nabu_beam_search_opts *o) {
  BeamGeo g;
  return beam_geo(d, &g) || beam_opts(&g, o) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_multi_beam_search_ex(const nabu_multi_beam_desc *d, const float *const *values,
                                                 const int32_t *const *enc_len, const nabu_speller_multi_params *p,
                                                 const nabu_beam_search_opts *o, int32_t *sequences, int32_t *lengths,
                                                 float *scores, float *const *alignments, int32_t *num_steps, void *ws,
                                                 size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g)) return e;
  if (int e = beam_opts(&g, o)) return e;
  return decode_multi(g, values, enc_len, p, sequences, lengths, scores, alignments, num_steps, ws, ws_bytes, stream,
                      o->ctc_logits, o->lm_table);
}

extern "C" size_t nabu_speller_multi_sample_ws_bytes(const nabu_multi_beam_desc *d) {
  BeamGeo g;
  return beam_geo(d, &g, true) ? 0 : beam_ws(g).total * 4;
}

extern "C" int nabu_speller_multi_sample(const nabu_multi_beam_desc *d, const float *const *values,
                                         const int32_t *const *enc_len, const nabu_speller_multi_params *p,
                                         unsigned long long seed, unsigned long long offset0, int32_t *sequences,
                                         int32_t *lengths, float *nll, float *const *alignments, int32_t *num_steps,
                                         void *ws, size_t ws_bytes, nabu_stream_t stream) {
  BeamGeo g;
  if (int e = beam_geo(d, &g, true)) return e;
  g.seed = seed; g.offset0 = offset0;
  return decode_multi(g, values, enc_len, p, sequences, lengths, nll, alignments, num_steps, ws, ws_bytes, stream);
}
