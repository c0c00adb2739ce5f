"""CTC prefix scoring restated in NumPy (importable without a GPU): the recurrences of nabu_ctc_prefix_prepare /
_score / _advance (include/nabu_hip.h) in float64 or, by the dtype argument, with every operation in float32 — the
measure of what float32 log-space arithmetic can deliver on a case (tests/ctc_cases.py: judge uses the CTC oracle the
same way).  enumerate_prefixes() is the independent check of the restatement itself: all C^T paths.

A beam is a dict of arrays: state [B,W,T,2] (r_n, r_b), psi [B,W], last [B,W] (-1: the empty hypothesis)."""
import itertools

import numpy as np

NEG = -1e30          # log 0, the finite stand-in of the kernels


def _lse(a, b):
    m, n = np.maximum(a, b), np.minimum(a, b)
    return m + np.log1p(np.exp(n - m))


def log_softmax(logits, dtype=np.float64):
    """y [.., C] and the normalisers (mx, lz) the prepare kernel stores: y = (x - mx) - lz"""
    x = np.asarray(logits).astype(dtype)
    mx = x.max(-1, keepdims=True)
    lz = np.log(np.exp(x - mx).sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    return (x - mx) - lz, mx[..., 0], lz[..., 0]


def prepare(logits, enc_len, W, dtype=np.float64):
    """(y [B,T,C], beam of the empty hypothesis in all W slots)"""
    y, _, _ = log_softmax(logits, dtype)
    B, T, C = y.shape
    state = np.full((B, W, T, 2), NEG, dtype)
    for b in range(B):
        a = dtype(0)
        for t in range(min(max(int(enc_len[b]), 0), T)):
            a = dtype(a + y[b, t, C - 1])
            state[b, :, t, 1] = max(a, dtype(NEG))
    return y, dict(state=state, psi=np.zeros((B, W), dtype), last=np.full((B, W), -1, np.int32))


def _phi(st, last, C, t):
    """phi_t [C-1] of a hypothesis with state st [T,2]: from frame t-1"""
    both = _lse(st[t - 1, 0], st[t - 1, 1])
    phi = np.full(C - 1, both, st.dtype)
    if last >= 0:
        phi[last] = st[t - 1, 1]
    return phi


def psi_all(y, Tb, st, last):
    """psi(g.c) for every class c of one hypothesis (c = C-1: psi(g.eos)), floored at NEG"""
    dtype = y.dtype.type
    C = y.shape[1]
    out = np.full(C, NEG, dtype)
    if Tb == 0:
        out[C - 1] = 0 if last < 0 else NEG
        return out
    v = y[0, :C - 1].copy() if last < 0 else np.full(C - 1, NEG, dtype)
    for t in range(1, Tb):
        v = _lse(v, _phi(st, last, C, t) + y[t, :C - 1])
    out[:C - 1] = v
    out[C - 1] = _lse(st[Tb - 1, 0], st[Tb - 1, 1])
    return np.maximum(out, dtype(NEG))


def extend(y, Tb, st, last, c):
    """(state [T,2], psi) of g.c for a label c != blank"""
    dtype = y.dtype.type
    T, C = y.shape
    new = np.full((T, 2), NEG, dtype)
    psi = dtype(NEG)
    if Tb > 0:
        rn, rb = (y[0, c] if last < 0 else dtype(NEG)), dtype(NEG)
        psi = rn
        new[0] = (rn, rb)
        for t in range(1, Tb):
            f = st[t - 1, 1] if c == last else _lse(st[t - 1, 0], st[t - 1, 1])
            n_rn = max(dtype(_lse(rn, f) + y[t, c]), dtype(NEG))
            n_rb = max(dtype(_lse(rb, rn) + y[t, C - 1]), dtype(NEG))
            psi = dtype(_lse(psi, dtype(f + y[t, c])))
            rn, rb = n_rn, n_rb
            new[t] = (rn, rb)
    return new, max(psi, dtype(NEG))


def score(y, enc_len, beam, finished=None):
    """delta [B,W,C] = psi(g.c) - psi(g); the row of a finished beam is zero"""
    B, W = beam['psi'].shape
    T, C = y.shape[1:]
    delta = np.zeros((B, W, C), y.dtype)
    with np.errstate(over='ignore', under='ignore'):
        for b in range(B):
            Tb = min(max(int(enc_len[b]), 0), T)
            for w in range(W):
                if finished is not None and finished[b, w]:
                    continue
                delta[b, w] = psi_all(y[b], Tb, beam['state'][b, w], int(beam['last'][b, w])) - beam['psi'][b, w]
    return delta


def advance(y, enc_len, beam, parent, stay, pred):
    """the beam of the survivors"""
    B, W = beam['psi'].shape
    T, C = y.shape[1:]
    new = dict(state=np.empty_like(beam['state']), psi=np.empty_like(beam['psi']), last=np.empty_like(beam['last']))
    with np.errstate(over='ignore', under='ignore'):
        for b in range(B):
            Tb = min(max(int(enc_len[b]), 0), T)
            for k in range(W):
                p, c = int(parent[b, k]), int(pred[b, k])
                st, last = beam['state'][b, p], int(beam['last'][b, p])
                if stay[b, k] or c == C - 1:
                    new['state'][b, k], new['last'][b, k] = st, last
                    new['psi'][b, k] = beam['psi'][b, p] if stay[b, k] else psi_all(y[b], Tb, st, last)[C - 1]
                else:
                    new['state'][b, k], new['psi'][b, k] = extend(y[b], Tb, st, last, c)
                    new['last'][b, k] = c
    return new


def prefix_state(y, Tb, g):
    """(state, psi, last) of the hypothesis g (a tuple of labels) of one utterance y [T,C], from the empty one"""
    dtype = y.dtype.type
    T, C = y.shape
    st = np.full((T, 2), NEG, dtype)
    a = dtype(0)
    for t in range(Tb):
        a = dtype(a + y[t, C - 1])
        st[t, 1] = a
    psi, last = dtype(0), -1
    for c in g:
        st, psi = extend(y, Tb, st, last, c)
        last = c
    return st, psi, last


def enumerate_prefixes(y, max_len):
    """{g: (log P(labelling starts with g), log P(labelling == g))} for every g up to max_len labels, by walking all
    C^T paths of y [T,C] (float64)"""
    T, C = y.shape
    start, exact = {}, {}
    for path in itertools.product(range(C), repeat=T):
        p = float(np.exp(sum(y[t, k] for t, k in enumerate(path))))
        lab = tuple(k for i, k in enumerate(path) if k != C - 1 and (i == 0 or k != path[i - 1]))
        for n in range(min(len(lab), max_len) + 1):
            start[lab[:n]] = start.get(lab[:n], 0.0) + p
        if len(lab) <= max_len:
            exact[lab] = exact.get(lab, 0.0) + p
    logp = lambda v: np.log(v) if v > 0 else -np.inf
    keys = [g for n in range(max_len + 1) for g in itertools.product(range(C - 1), repeat=n)]
    return {g: (logp(start.get(g, 0.0)), logp(exact.get(g, 0.0))) for g in keys}
