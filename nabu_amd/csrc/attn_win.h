// attn_win.h — the chunk window of the attention, shared by self_attn.hip and self_attn_bf16.hip (nabu_self_attn_win_* /
// nabu_self_attn_bf16_win_*, include/nabu_hip.h).
//
// THE WINDOW.  With chunk C >= 1 and left chunks Lc >= -1, query i of an utterance of length len sees key j iff
// lo(i) <= j < hi(i), hi(i) = min(len, (i / C + 1) C), lo(i) = 0 if Lc < 0, else max(0, (i / C - Lc) C): its own chunk
// and Lc chunks to its left (all of them when Lc < 0).  Both bounds are monotone in i and lo(i) <= i < hi(i).
// Read from the key's side: key j is seen by the queries qlo(j) <= i < qhi(j), qlo(j) = (j / C) C,
// qhi(j) = len if Lc < 0, else min(len, (j / C + Lc + 1) C).
//
// A lane computes its interval ONCE, in the prologue (one integer division by the runtime C), as a start and a span;
// the predicate per score is then one subtract and one unsigned compare, (unsigned)(j - start) < span: what the plain
// kernels spend on j < len.
//
// NO OVERFLOW: the host clamps C to T and turns an Lc that reaches past frame 0 for every query into -1, so C <= T,
// Lc C < T, and every product below is formed from a value below T; the chunk's end is compared as a distance.
#pragma once
#include "common.h"

namespace nabu {

struct AttnWin {                                 // rides at the end of the kernels' argument structs, after AttnDrop
  int chunk, left;                               // read by the WIN instantiations only
};

// the refusals the window entry points add to the dropout ones', and the clamped window
inline int attn_win_args(const char *what, int T, int chunk, int left_chunks, AttnWin *w) {
  NABU_CHECK_ARG(chunk >= 1, "%s: chunk = %d, must be at least 1", what, chunk);
  NABU_CHECK_ARG(left_chunks >= -1, "%s: left_chunks = %d, must be -1 (all chunks to the left) or at least 0", what,
                 left_chunks);
  const int Tc = T > 1 ? T : 1;
  w->chunk = chunk < Tc ? chunk : Tc;                                      // C >= T is C = T
  w->left = left_chunks >= (Tc - 1) / w->chunk ? -1 : left_chunks;         // the last chunk's window reaches frame 0
  return 0;
}

struct WinSpan {
  int start;
  unsigned span;
  __device__ __forceinline__ bool has(int j) const { return (unsigned)(j - start) < span; }
  __device__ __forceinline__ int end() const { return start + (int)span; }
};

// end of the stretch of `n` frames starting at `from` (a chunk boundary below len), cut at len
__device__ __forceinline__ int win_cut(int from, int n, int len) { return len - from > n ? from + n : len; }

// the keys query i < len sees
__device__ __forceinline__ WinSpan win_keys(const AttnWin &w, int i, int len) {
  const int own = i / w.chunk * w.chunk;
  const int lo = w.left < 0 ? 0 : max(0, own - w.left * w.chunk);
  return {lo, (unsigned)(win_cut(own, w.chunk, len) - lo)};
}

// the queries that see key j < len
__device__ __forceinline__ WinSpan win_queries(const AttnWin &w, int j, int len) {
  const int own = j / w.chunk * w.chunk;
  const int hi = w.left < 0 ? len : win_cut(own, (w.left + 1) * w.chunk, len);
  return {own, (unsigned)(hi - own)};
}

}  // namespace nabu

// one launch of an attention kernel K<dk, DROP, WIN>: dk 32 or 64, DROP when a mask is given and keep < 1, WIN when a window is given
#define ATTN_LAUNCH(K, dk, drop, win, grid, s, a)                                                              \
  do {                                                                                                           \
    if (dk == 64) {                                                                                              \
      if (win) { if (drop) hipLaunchKernelGGL((K<64, true, true>), grid, dim3(256), 0, s, a);                  \
                 else hipLaunchKernelGGL((K<64, false, true>), grid, dim3(256), 0, s, a); }                     \
      else if (drop) hipLaunchKernelGGL((K<64, true, false>), grid, dim3(256), 0, s, a);                        \
      else hipLaunchKernelGGL((K<64, false, false>), grid, dim3(256), 0, s, a);                                 \
    } else {                                                                                                     \
      if (win) { if (drop) hipLaunchKernelGGL((K<32, true, true>), grid, dim3(256), 0, s, a);                  \
                 else hipLaunchKernelGGL((K<32, false, true>), grid, dim3(256), 0, s, a); }                     \
      else if (drop) hipLaunchKernelGGL((K<32, true, false>), grid, dim3(256), 0, s, a);                        \
      else hipLaunchKernelGGL((K<32, false, false>), grid, dim3(256), 0, s, a);                                 \
    }                                                                                                            \
  } while (0)
