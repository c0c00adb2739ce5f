"""CTC prefix beam search with a label n-gram, restated as a search over a dictionary of prefixes (plain NumPy float64;
importable without a GPU): the reference of nabu_ctc_beam_search_lm.

Scorer semantics (TensorFlow's GetStateExpansionScore / GetStateEndExpansionScore, alpha = lm_weight, beta =
insertion_bonus).  A prefix g (a tuple of labels, NOT merged) holds (total, blank, label) log-probabilities.  Per frame,
with y the frame's log-softmax and `old` the values before the frame:
  (1) a prefix in the beam:  label = old.label, and if its parent g[:-1] was in the beam at the previous frame
          label = lse(label, prev + term(g)),  prev = parent.old.blank if g[-1] == parent[-1] else parent.old.total;
      then label += y[g[-1]] (the root has no label part);  blank = old.total + y[blank];  total = lse(blank, label).
      Staying in g — the blank, and the repeated-label self loop old.label — carries NO term.
  (2) g.c for every label c, unless g.c is itself in the beam:  total = label = y[c] + (prev + term(g.c)),
      prev = old.blank if c == g[-1] else old.total.
  term(g.c) = alpha * logp[ctx(g), c] + beta: what a transition that APPENDS c to g carries.
  (3) the beam_width best live candidates by (total descending, insertion order: the prefixes of (1) in beam order, then
      the expansions by (prefix, label)).
After the last frame the beam is ranked by total + alpha * logp[ctx(g), C-1]; that value is the result's `total`.
merge_repeated collapses equal neighbours of the OUTPUT labelling; the LM context is the unmerged prefix.

details=True reports what tests/decode_cases.py judges admissibility by (select_gap, select_ties, order_gap, top_gap,
max_abs_total, as oracle.decode_oracle.ctc_beam_search defines them; top_gap and max_abs_total include the final
ranking with the end term)."""
import numpy as np

NEG = -np.inf


def _lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def _ctx(g, C, n):
    """context index of prefix g: its last n-1 symbols, padded with the boundary in front, most recent least significant"""
    h = ((C - 1,) * (n - 1) + tuple(g))[len(g):] if n > 1 else ()
    idx = 0
    for s in h:
        idx = idx * C + s
    return idx


def _merge(g, merge_repeated):
    out, prev = [], -1
    for c in g:
        if not merge_repeated or c != prev:
            out.append(int(c))
        prev = c
    return out


def search(logits, logp, order, alpha, beta, beam_width=100, merge_repeated=True, details=False, term_on_self_loop=False):
    """One utterance: logits [T,C] (T its length, possibly 0), logp [C^(order-1), C] the table of log-probabilities.
    Returns the labels of the best prefix, or with details=True a dict (see the module's docstring; also `beam`: the
    final beam as [(unmerged labels, fused total)] best first).
    term_on_self_loop=True is a deliberately WRONG variant — the term is also added on the repeated-label self loop — for
    building cases in which that mistake would change the winner."""
    logits = np.asarray(logits, np.float64)
    T, C = logits.shape
    blank, n = C - 1, int(order)
    logp = np.asarray(logp, np.float64)
    assert logp.shape == (C ** (n - 1), C)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = logits - logits.max(1, keepdims=True) if T else logits
        y = y - np.log(np.exp(y).sum(1, keepdims=True)) if T else y

    def term(g):        # g non-empty: entering g from g[:-1]
        return alpha * logp[_ctx(g[:-1], C, n), g[-1]] + beta

    beam = [()]                                 # best first
    prob = {(): (0.0, 0.0, NEG)}                # prefix -> (total, blank, label)
    select_gap = order_gap = np.inf
    select_ties, max_abs = 0, 0.0
    for t in range(T):
        old = prob
        cands = []                              # (prefix, (total, blank, label)) in insertion order
        for g in beam:
            ot, ob, ol = old[g]
            lab = ol
            if g:
                if term_on_self_loop and lab != NEG:
                    lab = lab + term(g)
                par = g[:-1]
                if par in old:
                    pt, pb, _ = old[par]
                    prev = pb if (par and par[-1] == g[-1]) else pt
                    lab = _lse(lab, prev + term(g))
                lab = lab + y[t, g[-1]]
            blk = ot + y[t, blank]
            cands.append((g, (_lse(blk, lab), blk, lab)))
        for g in beam:
            ot, ob, _ = old[g]
            if not ot > NEG:
                continue
            for c in range(C - 1):
                h = g + (c,)
                if h in old:
                    continue                    # already in the beam, updated above
                prev = ob if (g and g[-1] == c) else ot
                sc = y[t, c] + (prev + term(h))
                cands.append((h, (sc, NEG, sc)))
        live = [(i, g, p) for i, (g, p) in enumerate(cands) if p[0] > NEG]
        live.sort(key=lambda e: (-e[2][0], e[0]))
        keep, drop = live[:beam_width], live[beam_width:]
        if live:
            max_abs = max(max_abs, max(abs(p[0]) for _, _, p in live))
            tot = [p[0] for _, _, p in keep]
            for d in np.diff(tot):
                if d != 0:
                    order_gap = min(order_gap, -d)
            if drop:
                thr, dr = tot[-1], [p[0] for _, _, p in drop]
                if max(dr) == thr:
                    select_ties += 1
                    near = [v - thr for v in tot if v != thr] + [thr - v for v in dr if v != thr]
                else:
                    near = [thr - max(dr)]
                if near:
                    select_gap = min(select_gap, min(near))
        beam = [g for _, g, _ in keep]
        prob = {g: p for _, g, p in keep}
        if not beam:
            break
    final = sorted(((prob[g][0] + alpha * logp[_ctx(g, C, n), blank], i, g) for i, g in enumerate(beam)),
                   key=lambda e: (-e[0], e[1]))
    labels = _merge(final[0][2], merge_repeated) if final else []
    if not details:
        return labels
    if final:
        max_abs = max(max_abs, max(abs(v) for v, _, _ in final))
    return dict(labels=labels, total=final[0][0] if final else NEG, beam=[(list(g), v) for v, _, g in final],
                select_gap=float(select_gap), select_ties=select_ties, order_gap=float(order_gap),
                top_gap=float(final[0][0] - final[1][0]) if len(final) > 1 else np.inf, max_abs_total=max_abs)


def search_batch(logits, lens, logp, order, alpha, beta, beam_width=100, merge_repeated=True, **kw):
    """details of every utterance of a batch [B,T,C]; lengths clamped to [0, T] as the kernel clamps them"""
    T = logits.shape[1]
    return [search(np.asarray(logits[b][:int(np.clip(lens[b], 0, T))]), logp, order, alpha, beta, beam_width,
                   merge_repeated, details=True, **kw) for b in range(len(lens))]
