"""The alignment-length synchronous beam search of the RNN transducer, restated in NumPy (importable without a GPU):
the yardstick of nabu_transducer_beam_step (include/nabu_hip.h has the definition; this file follows it rule by rule).

At iteration i every active hypothesis with u labels sits at frame i - u, so one joint evaluation per hypothesis and
iteration does the whole beam.  Hypotheses that spell the same labels meet at the same lattice node in the same
iteration and their probabilities are added (the merge); with nothing pruned the final score of y is log P(y | x), what
brute_force_nll of tests/transducer_ref.py enumerates.  beam_search(merge=False) leaves the merge out: the beam may then
hold one label sequence several times, as a search that cannot add would."""
import numpy as np

from tests.transducer_ref import logadd


def _log_probs(x, dtype):
    m = x.max()
    return ((x - m) - np.log(np.exp(x - m).sum(dtype=dtype))).astype(dtype)


def _empty_beam(W, S, C, dtype):
    return dict(ids=np.full((W, S), -1, np.int32), out_len=np.full(W, -1, np.int32), score=np.full(W, -np.inf, dtype),
                parent=np.arange(W, dtype=np.int32), emit=np.zeros(W, np.int32), last_id=np.full(W, C - 1, np.int32))


def _finals_arrays(finals, W, S, dtype):
    ids, ln, sc = np.full((W, S), -1, np.int32), np.full(W, -1, np.int32), np.full(W, -np.inf, dtype)
    for j, (y, s) in enumerate(finals):
        ids[j, :len(y)], ln[j], sc[j] = y, len(y), s
    return dict(fin_ids=ids, fin_len=ln, fin_score=sc)


def _offer(finals, y, s, W):
    """behind the finals of equal score; what falls past W is dropped"""
    at = len(finals)
    while at > 0 and finals[at - 1][1] < s:
        at -= 1
    finals.insert(at, (tuple(y), s))
    del finals[W:]


def search_one(f, enc_len, S, W, g_fn, iters, dtype=np.float64, merge=True):
    """one utterance: f [T,C], g_fn(labels tuple) -> [C].  Returns (finals [(labels, score)], trace, stats)"""
    T, C = f.shape
    blank = C - 1
    el = min(max(int(enc_len), 0), T)
    active = [((), dtype(0))] if el > 0 else []
    finals = [] if el > 0 else [((), dtype(0))]
    trace, stats = [], dict(merges=0, shrinks=0, margin=np.inf, capped=0, evals=0)
    for i in range(iters):
        n = len(active)
        v = np.full((max(n, 1), C), np.nan, dtype)             # NaN: no such candidate
        for w, (y, s) in enumerate(active):
            t = i - len(y)
            assert 0 <= t < el
            lp = _log_probs((f[t].astype(dtype) + np.asarray(g_fn(y)).astype(dtype)).astype(dtype), dtype)
            stats['evals'] += 1
            if len(y) == S:
                v[w, blank] = s + lp[blank]
                stats['capped'] += 1
            else:
                v[w] = s + lp
        if merge:
            where = {y: w for w, (y, _) in enumerate(active)}
            assert len(where) == n                             # active hypotheses are pairwise distinct
            for a, (y, _) in enumerate(active):
                c = where.get(y[:-1]) if y else None
                if c is not None:
                    k = y[-1]
                    v[a, blank] = logadd(v[a, blank], v[c, k])
                    v[c, k] = np.nan
                    stats['merges'] += 1
        flat = v[:n].reshape(-1) if n else np.zeros(0, dtype)
        live = np.flatnonzero(~np.isnan(flat))
        order = live[np.lexsort((live, -flat[live]))]          # value, largest first; equal values by flat index
        top = flat[order[:W + 1]]
        if len(top) > 1:
            stats['margin'] = min(stats['margin'], float(np.min(top[:-1] - top[1:])))
        beam = _empty_beam(W, S, C, dtype)
        new = []
        for idx in order[:W]:
            w, k = divmod(int(idx), C)
            y, _ = active[w]
            if k == blank and i - len(y) + 1 == el:
                _offer(finals, y, flat[idx], W)
                continue
            slot = len(new)
            ny = y if k == blank else y + (k,)
            new.append((ny, flat[idx]))
            beam['ids'][slot, :len(ny)], beam['out_len'][slot], beam['score'][slot] = ny, len(ny), flat[idx]
            beam['parent'][slot], beam['emit'][slot] = w, int(k != blank)
            beam['last_id'][slot] = k
        if len(new) < n:
            stats['shrinks'] += 1
        active = new
        beam.update(_finals_arrays(finals, W, S, dtype))
        trace.append(beam)
    return list(finals), trace, stats


def beam_search(f, enc_len, S, W, g_fn, dtype=np.float64, iters=None, merge=True):
    """The search over a batch: f [B,T,C], g_fn(b, labels tuple) -> the prediction logits [C] of that history.  Runs
    `iters` iterations (T + S when None: no utterance has an active hypothesis after that) and returns
      finals   per utterance [(labels, score)], best first;
      trace    per iteration {ids [B,W,S], out_len, score, parent, emit, last_id [B,W], fin_ids, fin_len, fin_score};
      merges   per utterance, how many candidates were added to another;
      shrinks  per utterance, the iterations after which the beam held fewer hypotheses than before;
      margin   the least gap between neighbours among the first W + 1 ordered candidates, over everything;
      capped   per utterance, the evaluations of a hypothesis that held S labels (it continues by blanks)."""
    B, T, C = f.shape
    iters = T + S if iters is None else iters
    per = [search_one(f[b], enc_len[b], S, W, lambda y, b=b: g_fn(b, y), iters, dtype, merge) for b in range(B)]
    trace = [{k: np.stack([p[1][i][k] for p in per]) for k in per[0][1][i]} for i in range(iters)]
    return dict(finals=[p[0] for p in per], trace=trace, merges=[p[2]['merges'] for p in per],
                shrinks=[p[2]['shrinks'] for p in per], margin=min(p[2]['margin'] for p in per),
                capped=[p[2]['capped'] for p in per])


def best(finals, S):
    """(ids [B,S] padded with -1, lengths, scores) of every utterance's best final"""
    ids = np.full((len(finals), S), -1, np.int32)
    for b, fin in enumerate(finals):
        ids[b, :len(fin[0][0])] = fin[0][0]
    return ids, np.array([len(fin[0][0]) for fin in finals], np.int32), np.array([fin[0][1] for fin in finals])
