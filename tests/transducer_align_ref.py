"""Forced alignment with the transducer, restated in NumPy (importable without a GPU): the yardstick of
nabu_transducer_align (include/nabu_hip.h).

align() is the definition of the header evaluated in `dtype`: float64 is the reference, float32 the measure of what
float32 arithmetic can deliver on a case.  Either way h = f + g is ONE float32 addition, as the header says; the rest
runs in `dtype`.  The tie rule is the header's: the label move wins only if strictly greater, and the backtrace runs
from the final blank's node (T_b-1, U_b) to (0,0).  tests/test_transducer_align_ref.py holds viterbi() to an
enumeration of every monotone path (best_paths).

grid_case() draws the exact grid of the issue: one class d = C-2 that no label names has f = 256 and g = 0, every
other logit is a multiple of 0.25 in [-1, 1].  Then exp(h - mx) underflows to exactly 0 for every class but d in
float32 and adds less than half an ulp to 1 in float64: lz = 0, every lb and ly is a multiple of 0.25 near -256, and
every partial sum of at most 2^14 of them is exact in float32.  Both precisions return the same path and score, and the
many equal values make ties genuine."""
import itertools

import numpy as np

from tests import transducer_cases as tc
from tests.transducer_ref import NEG, utterance_ok

GRID_VALUES = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32)


def terms(f, g, lab, dtype=np.float64):
    """(lb, ly) [T,U1] of one utterance: f [T,C], g [U1,C] float32, lab [U1-1].  ly[:, U] is unreachable"""
    T, C = f.shape
    U1 = g.shape[0]
    assert f.dtype == np.float32 and g.dtype == np.float32 and len(lab) == U1 - 1
    h = (f[:, None, :] + g[None, :, :]).astype(dtype)                  # (one float32 addition)
    m = h.max(axis=2, keepdims=True)
    with np.errstate(under='ignore'):
        lz = np.log(np.exp(h - m).astype(dtype).sum(axis=2, keepdims=True, dtype=dtype)).astype(dtype)
    lp = ((h - m) - lz).astype(dtype)
    lb = lp[:, :, C - 1]
    ly = np.full((T, U1), NEG, dtype)
    if U1 > 1:
        ly[:, :U1 - 1] = lp[:, np.arange(U1 - 1), np.asarray(lab, np.int64)]
    return np.ascontiguousarray(lb), ly


def viterbi(lb, ly):
    """The recursion in the dtype of lb / ly, anti-diagonal by anti-diagonal.  Returns (v [T,U1], label_move [T,U1] bool,
    ties): v is the larger candidate, label_move[t,u] says the label move made it (strictly greater; a move that does
    not exist — the label move in column 0, the blank move at frame 0 — is the unreachable -1e30 and is never TAKEN,
    whatever the values say: with -inf terms the back-pointers still name a path inside the lattice), ties counts the nodes with BOTH
    predecessors whose candidates were equal."""
    T, U1 = lb.shape
    dtype = lb.dtype.type
    neg = dtype(NEG)
    v = np.full((T, U1), neg, dtype)
    move = np.zeros((T, U1), bool)
    v[0, 0] = 0
    ties = 0
    for d in range(1, T + U1 - 1):
        u = np.arange(max(0, d - T + 1), min(d, U1 - 1) + 1)
        t = d - u
        tp, up = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        stay = np.where(t >= 1, v[tp, u] + lb[tp, u], neg)
        emit = np.where(u >= 1, v[t, up] + ly[t, up], neg)
        assert stay.dtype == lb.dtype and emit.dtype == lb.dtype
        v[t, u] = np.where(emit > stay, emit, stay)
        move[t, u] = (u >= 1) & ((t == 0) | (emit > stay))          # among the moves that exist
        ties += int(np.count_nonzero((t >= 1) & (u >= 1) & (emit == stay)))
    return v, move, ties


def backtrace(move):
    """(state [T], frame [U]) of the path the back-pointers name, from (T-1, U) to (0,0)"""
    T, U1 = move.shape
    state, frame = np.zeros(T, np.int32), np.zeros(U1 - 1, np.int32)
    t, u = T - 1, U1 - 1
    state[t] = u
    while (t, u) != (0, 0):
        if move[t, u]:
            u -= 1
            frame[u] = t
        else:
            t -= 1
            state[t] = u
        assert t >= 0 and u >= 0
    return state, frame


def path_terms(lb, ly, frame):
    """the T + U terms of the path that emits label i at frame[i], in path order, and conf [U] = ly[frame[i], i]"""
    T, U1 = lb.shape
    out, conf = [], np.zeros(U1 - 1, lb.dtype)
    u = 0
    for t in range(T):
        while u < U1 - 1 and frame[u] == t:
            out.append(ly[t, u])
            conf[u] = ly[t, u]
            u += 1
        out.append(lb[t, u])
    assert u == U1 - 1, 'frame is not a path'
    return np.array(out, lb.dtype), conf


def align(f, g, enc_len, labels, label_len, dtype=np.float64):
    """(state [B,T] int32, frame [B,U1-1] int32, conf [B,U1-1], score [B], status, ties [B]): the definition of
    nabu_transducer_align in `dtype`; score is the recursion's value v[T_b-1,U_b] + lb[T_b-1,U_b]"""
    B, T, C = f.shape
    U1 = g.shape[1]
    state, frame = np.full((B, T), -1, np.int32), np.full((B, U1 - 1), -1, np.int32)
    conf, score = np.zeros((B, U1 - 1), dtype), np.full(B, -np.inf, dtype)
    ties = np.zeros(B, np.int64)
    status = 0
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(label_len[b])
        lab = labels[b] if labels is not None else np.zeros(0, np.int64)
        if not utterance_ok(Tb, Ub, lab, T, U1, C):
            status = status or b + 1
            continue
        lb, ly = terms(f[b, :Tb], g[b, :Ub + 1], lab[:Ub], dtype)
        v, move, ties[b] = viterbi(lb, ly)
        state[b, :Tb], frame[b, :Ub] = backtrace(move)
        _, conf[b, :Ub] = path_terms(lb, ly, frame[b, :Ub])
        score[b] = v[Tb - 1, Ub] + lb[Tb - 1, Ub]
    return state, frame, conf, score, status, ties


def check_path(state, frame, Tb, Ub, T, U):
    """'' if (state [T], frame [U]) is a valid path of an utterance with Tb frames and Ub labels, else what is wrong"""
    s, fr = np.asarray(state), np.asarray(frame)
    if not (np.all(s[Tb:] == -1) and np.all(fr[Ub:] == -1)):
        return 'tails are not -1'
    s, fr = s[:Tb], fr[:Ub]
    if np.any(s < 0) or np.any(s > Ub) or np.any(np.diff(s) < 0) or s[-1] != Ub:
        return 'state is not a non-decreasing walk to U_b'
    want = np.array([int(np.argmax(s > i)) for i in range(Ub)], np.int64)          # the first t with state[t] > i
    if not np.array_equal(fr, want):
        return 'frame is not the first t with state[t] > i'
    return ''


def path_values(f, g, enc_len, labels, label_len, frame):
    """float64 values of the paths a result names: (score [B], conf [B,U1-1], sum |terms| [B]); rows with frame[0] < 0
    although they have labels (rejected) get nan"""
    B, U1 = f.shape[0], g.shape[1]
    score, conf, sabs = np.full(B, np.nan), np.zeros((B, U1 - 1)), np.zeros(B)
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(label_len[b])
        if not utterance_ok(Tb, Ub, labels[b] if labels is not None else [], f.shape[1], U1, f.shape[2]):
            continue
        lb, ly = terms(f[b, :Tb], g[b, :Ub + 1], labels[b, :Ub] if Ub else np.zeros(0, np.int64))
        x, conf[b, :Ub] = path_terms(lb, ly, frame[b, :Ub])
        score[b], sabs[b] = x.sum(), np.abs(x).sum()
    return score, conf, sabs


def best_paths(lb, ly):
    """Every monotone path of one utterance enumerated (the T-1 blanks before the final one and the U labels in all
    C(T+U-1, U) orders), each summed in path order: (best value, [frame tuples of the paths that reach it], count)"""
    T, U1 = lb.shape
    U = U1 - 1
    best, arg, count = None, [], 0
    for emits in itertools.combinations(range(T + U - 1), U):
        t = u = 0
        total = lb.dtype.type(0)
        frame = []
        for step in range(T + U - 1):
            if step in emits:
                total = total + ly[t, u]
                frame.append(t)
                u += 1
            else:
                total = total + lb[t, u]
                t += 1
        assert (t, u) == (T - 1, U)
        total = total + lb[t, u]
        count += 1
        if best is None or total > best:
            best, arg = total, [tuple(frame)]
        elif total == best:
            arg.append(tuple(frame))
    return best, arg, count


def tie_rule_choice(paths):
    """Of equally good paths the tie rule names ONE.  The backtrace prefers the blank move at every node it stands on,
    i.e. it leaves label U-1 as early as any best path does, then label U-2 given that, and so on: the smallest
    (frame[U-1], frame[U-2], .., frame[0])"""
    return min(paths, key=lambda fr: tuple(reversed(fr)))


# ------------------------------------------------------------------------------------------------ cases
def grid_case(shape, seed=None):
    """(f, g, enc_len, labels, label_len) on the exact grid, with the lengths of transducer_cases.make_case (utterance 0
    full, the last with all Lmax labels, utterance 1 without labels when B >= 3).  Needs C >= 3: the spare class"""
    B, T, C, Lmax = shape
    assert C >= 3
    c = tc.make_case(B, T, C, Lmax, 'random', tc.seed_of(*shape) if seed is None else seed)
    rng = np.random.default_rng([tc.seed_of(*shape) if seed is None else seed, 7])
    f = GRID_VALUES[rng.integers(0, len(GRID_VALUES), (B, T, C))]
    g = GRID_VALUES[rng.integers(0, len(GRID_VALUES), (B, Lmax + 1, C))]
    f[:, :, C - 2] = 256.0
    g[:, :, C - 2] = 0.0
    labels = (c.labels % (C - 2)).astype(np.int32)                    # never the spare class, never the blank
    return np.ascontiguousarray(f), np.ascontiguousarray(g), c.enc_len.copy(), labels, c.label_len.copy()


def constant_case(B, T, C, Lmax):
    """f = g = 0: every path of an utterance has the same value bit for bit; the tie rule alone decides"""
    rng = np.random.default_rng(5)
    enc_len = np.full(B, T, np.int32)
    label_len = np.full(B, Lmax, np.int32)
    if B > 1:
        enc_len[1:] = rng.integers(max(1, T // 2), T + 1, B - 1)
        label_len[1:] = rng.integers(0, Lmax + 1, B - 1)
    labels = rng.integers(0, C - 1, (B, Lmax)).astype(np.int32)
    return np.zeros((B, T, C), np.float32), np.zeros((B, Lmax + 1, C), np.float32), enc_len, labels, label_len
