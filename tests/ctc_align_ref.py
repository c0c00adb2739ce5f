"""Forced alignment with a CTC model, restated in NumPy (importable without a GPU): the yardstick of nabu_ctc_align.

align(..., dtype) is the definition in include/nabu_hip.h word for word — a max-plus sweep over the label lattice on
the RAW logits with back-pointers, a tie keeping the smaller move, the end rule, then the log-softmax terms along the
path.  dtype = float64 is the reference; dtype = float32 is its twin: the same code in the kernel's number format,
the measure of what float32 can deliver on a case (the role ctc_cases.Case.oracle's float32 run has for the loss).

brute_force() enumerates every label string of a tiny problem and is what the float64 restatement itself is held to
(tests/test_ctc_align_ref.py).  path_values() evaluates a GIVEN path in float64: what a kernel's score and conf are
compared with."""
import itertools

import numpy as np

NEG = -1e30             # unreachable: CTC_NEG of csrc/ctc.hip


def extended(labels, blank):
    ext = np.full(2 * len(labels) + 1, blank, np.int64)
    ext[1::2] = labels
    return ext


def valid(labels, Tb, C):
    """ctc_kernel's test: every label in [0, C-1), Tb > 0, L + adjacent repeats <= Tb"""
    labels = np.asarray(labels, np.int64)
    if np.any(labels < 0) or np.any(labels >= C - 1) or Tb <= 0:
        return False
    return len(labels) + int(np.sum(labels[1:] == labels[:-1])) <= Tb


def viterbi(x, labels, dtype=np.float64):
    """x [Tb,C] raw logits, blank = C-1 -> (path [Tb] of lattice states, best raw score v[Tb-1][end]) in `dtype`"""
    x = np.asarray(x).astype(dtype)
    Tb, C = x.shape
    ext = extended(labels, C - 1)
    S = len(ext)
    neg = dtype(NEG)
    can_skip = np.zeros(S, bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(S, neg, dtype)
    v[0] = x[0, ext[0]]
    if S > 1:
        v[1] = x[0, ext[1]]
    bp = np.zeros((Tb, S), np.int8)
    for t in range(1, Tb):
        step = np.concatenate(([neg], v[:-1])).astype(dtype)
        skip = np.where(can_skip, np.concatenate(([neg, neg], v[:-2]))[:S], neg).astype(dtype)
        m = v.copy()
        k = np.zeros(S, np.int8)
        w = step > m                      # the step wins only if strictly greater than the stay
        m[w], k[w] = step[w], 1
        w = can_skip & (skip > m)         # the skip only if strictly greater than both
        m[w], k[w] = skip[w], 2
        v = (m + x[t, ext]).astype(dtype)
        bp[t] = k
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    best = v[s]
    path = np.zeros(Tb, np.int64)
    for t in range(Tb - 1, -1, -1):
        path[t] = s
        s -= int(bp[t, s])
    return path, best


def log_softmax_terms(x, classes, dtype=np.float64):
    """(x[t, c_t] - mx[t]) - lz[t], maximum and log-sum kept apart"""
    x = np.asarray(x).astype(dtype)
    mx = x.max(1)
    lz = np.log(np.exp(x - mx[:, None]).sum(1, dtype=dtype)).astype(dtype)
    return ((x[np.arange(len(classes)), classes] - mx) - lz).astype(dtype)


def segments(path, L):
    """[L,2]: first frame, last frame + 1 of every label state of a monotone path"""
    seg = np.full((L, 2), -1, np.int64)
    for i in range(L):
        at = np.flatnonzero(path == 2 * i + 1)
        seg[i] = (at[0], at[-1] + 1)
    return seg


def align(logits, logit_len, labels, label_len, dtype=np.float64):
    """-> state [B,T] int32, seg [B,Lmax,2] int32, conf [B,Lmax], score [B] (dtype), status (0 or 1 + first bad row)"""
    logits = np.asarray(logits)
    B, T, C = logits.shape
    Lmax = labels.shape[1]
    state = np.full((B, T), -1, np.int32)
    seg = np.full((B, Lmax, 2), -1, np.int32)
    conf = np.zeros((B, Lmax), dtype)
    score = np.zeros(B, dtype)
    status = 0
    for b in range(B):
        Tb = int(min(max(logit_len[b], 0), T))
        L = int(min(max(label_len[b], 0), Lmax))
        lab = np.asarray(labels[b, :L], np.int64)
        if not valid(lab, Tb, C):
            score[b] = -np.inf
            status = status or b + 1
            continue
        path, _ = viterbi(logits[b, :Tb], lab, dtype)
        terms = log_softmax_terms(logits[b, :Tb], extended(lab, C - 1)[path], dtype)
        state[b, :Tb] = path
        seg[b, :L] = segments(path, L)
        score[b] = terms.sum(dtype=dtype)
        for i in range(L):
            conf[b, i] = terms[seg[b, i, 0]:seg[b, i, 1]].mean(dtype=dtype)
    return state, seg, conf, score, status


def path_values(logits, logit_len, labels, label_len, state):
    """a GIVEN path in float64: (score [B], conf [B,Lmax], raw [B] = sum of the raw logits along it, sum|terms| [B],
    sum|raw logits| [B]); rows whose path starts with -1 are left at 0"""
    B, T, C = logits.shape
    Lmax = labels.shape[1]
    score, raw, sabs, rabs = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    conf = np.zeros((B, Lmax))
    for b in range(B):
        Tb, L = int(min(max(logit_len[b], 0), T)), int(min(max(label_len[b], 0), Lmax))
        if Tb <= 0 or state[b, 0] < 0:
            continue
        path = np.asarray(state[b, :Tb], np.int64)
        cls = extended(np.asarray(labels[b, :L], np.int64), C - 1)[path]
        x = logits[b, :Tb].astype(np.float64)
        terms = log_softmax_terms(x, cls)
        score[b], sabs[b] = terms.sum(), np.abs(terms).sum()
        picked = x[np.arange(Tb), cls]
        raw[b], rabs[b] = picked.sum(), np.abs(picked).sum()
        for i in range(L):
            at = path == 2 * i + 1
            if at.any():
                conf[b, i] = terms[at].mean()
    return score, conf, raw, sabs, rabs


def check_path(state_row, Tb, labels, T):
    """a valid path: starts in state 0 or 1, moves by 0, 1 or (between different labels) 2, ends in S-1 or S-2,
    -1 past Tb; returns a list of complaints"""
    L = len(labels)
    S = 2 * L + 1
    p = np.asarray(state_row[:Tb], np.int64)
    bad = []
    if not np.all(np.asarray(state_row[Tb:T]) == -1):
        bad.append('tail is not -1')
    if p.min() < 0 or p.max() >= S:
        return bad + ['state out of range']
    if p[0] > min(1, S - 1):
        bad.append('starts in state %d' % p[0])
    if p[-1] < S - 2:
        bad.append('ends in state %d of %d' % (p[-1], S))
    d = np.diff(p)
    if np.any(d < 0) or np.any(d > 2):
        bad.append('not monotone / jumps')
    for t in np.flatnonzero(d == 2):
        s = p[t + 1]
        if s % 2 == 0 or labels[s >> 1] == labels[(s >> 1) - 1]:
            bad.append('illegal skip into state %d at frame %d' % (s, t + 1))
    return bad


def collapse(classes, blank):
    """merge repeats, drop blanks"""
    out, prev = [], None
    for c in classes:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def brute_force(x, labels):
    """the best raw score over ALL C^T label strings that collapse to `labels` (None if there is none)"""
    Tb, C = x.shape
    best = None
    target = [int(l) for l in labels]
    for string in itertools.product(range(C), repeat=Tb):
        if collapse(string, C - 1) == target:
            sc = float(np.sum(x[np.arange(Tb), list(string)].astype(np.float64)))
            if best is None or sc > best:
                best = sc
    return best


def grid_logits(rng, shape):
    """multiples of 1/4 in [-8, 8]: every partial sum of a path is exact in float32, and ties are frequent"""
    return (rng.integers(-32, 33, shape) / 4.0).astype(np.float32)
