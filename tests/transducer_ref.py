"""RNN transducer with the additive joint, restated in NumPy (importable without a GPU): the yardstick of
nabu_transducer_loss_grad and nabu_transducer_greedy_step (include/nabu_hip.h).

loss_grad() is the definition of the header, evaluated in `dtype`: float64 is the reference, float32 the measure of
what float32 log-space arithmetic can deliver on a case (tests/transducer_cases.py: judge).  Here h [T,U1,C] IS
materialised, per utterance: this is the restatement, not the kernel.  tests/test_transducer_ref.py holds it to an
enumeration of every path (brute_force_nll) and to central differences.  greedy_search() is the lock-step greedy
search row by row."""
import itertools

import numpy as np

NEG = -1e30            # unreachable (TR_NEG of csrc/transducer.hip)


def logadd(a, b):
    m, n = np.maximum(a, b), np.minimum(a, b)
    return m + np.log1p(np.exp(n - m))


def utterance_ok(Tb, Ub, lab, T, U1, C):
    return 1 <= Tb <= T and 0 <= Ub <= U1 - 1 and all(0 <= int(l) < C - 1 for l in lab[:max(Ub, 0)])


def log_probs(f, g, dtype=np.float64):
    """log p(k | t,u) [T,U1,C] of one utterance: (h - max) - log sum exp(h - max), each node with its own maximum"""
    h = (f.astype(dtype)[:, None, :] + g.astype(dtype)[None, :, :]).astype(dtype)
    m = h.max(axis=2, keepdims=True)
    lz = np.log(np.exp(h - m).sum(axis=2, keepdims=True, dtype=dtype))
    return ((h - m) - lz).astype(dtype)


def lattice(lp, lab, dtype=np.float64):
    """(lb, ly, alpha, beta) [T,U1] of one utterance from its log-probabilities lp [T,U1,C] (U1 = len(lab) + 1)"""
    T, U1, C = lp.shape
    U = U1 - 1
    neg = dtype(NEG)
    lb = lp[:, :, C - 1]
    ly = np.full((T, U1), neg, dtype)
    if U:
        ly[:, :U] = lp[:, np.arange(U), np.asarray(lab[:U], np.int64)]
    alpha = np.full((T, U1), neg, dtype)
    beta = np.full((T, U1), neg, dtype)
    alpha[0, 0] = 0
    for d in range(1, T + U):                       # anti-diagonals; node (d-u, u)
        u = np.arange(max(0, d - T + 1), min(d, U) + 1)
        t = d - u
        stay = np.where(t >= 1, alpha[np.maximum(t - 1, 0), u] + lb[np.maximum(t - 1, 0), u], neg)
        emit = np.where(u >= 1, alpha[t, np.maximum(u - 1, 0)] + ly[t, np.maximum(u - 1, 0)], neg)
        alpha[t, u] = logadd(stay, emit)
    beta[T - 1, U] = lb[T - 1, U]
    for d in range(T + U - 2, -1, -1):
        u = np.arange(max(0, d - T + 1), min(d, U) + 1)
        t = d - u
        stay = np.where(t + 1 < T, beta[np.minimum(t + 1, T - 1), u], neg) + lb[t, u]
        emit = np.where(u + 1 <= U, beta[t, np.minimum(u + 1, U)], neg) + ly[t, u]
        beta[t, u] = logadd(stay, emit)
    return lb, ly, alpha, beta


def loss_grad(f, g, enc_len, labels, label_len, dtype=np.float64):
    """(nll [B], df [B,T,C], dg [B,U1,C], status) in `dtype`: the definition of nabu_transducer_loss_grad with
    grad_scale = 1.  An invalid utterance has nll 0 and zero gradients; status is 1 + the first such utterance."""
    B, T, C = f.shape
    U1 = g.shape[1]
    nll = np.zeros(B, dtype)
    df, dg = np.zeros((B, T, C), dtype), np.zeros((B, U1, C), dtype)
    status = 0
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(label_len[b])
        lab = labels[b] if labels is not None else np.zeros(0, np.int64)
        if not utterance_ok(Tb, Ub, lab, T, U1, C):
            status = status or b + 1
            continue
        lp = log_probs(f[b, :Tb], g[b, :Ub + 1], dtype)
        lb, ly, alpha, beta = lattice(lp, lab[:Ub], dtype)
        n = -beta[0, 0]
        nll[b] = n
        neg = dtype(NEG)
        bt = np.full((Tb, Ub + 1), neg, dtype)          # beta[t+1, u]; beta[Tb, Ub] reads as 0
        bt[:-1] = beta[1:]
        bt[Tb - 1, Ub] = 0
        bu = np.full((Tb, Ub + 1), neg, dtype)          # beta[t, u+1]
        bu[:, :-1] = beta[:, 1:]
        G = np.exp((alpha + beta) + n)[:, :, None] * np.exp(lp)
        G[:, :, C - 1] -= np.exp(((alpha + lb) + bt) + n)
        if Ub:
            G[:, np.arange(Ub), np.asarray(lab[:Ub], np.int64)] -= np.exp(((alpha + ly) + bu) + n)[:, :Ub]
        assert G.dtype == dtype
        df[b, :Tb] = G.sum(axis=1, dtype=dtype)
        dg[b, :Ub + 1] = G.sum(axis=0, dtype=dtype)
    return nll, df, dg, status


def brute_force_nll(f, g, lab):
    """-log of the sum over EVERY monotone path of one utterance (float64): the T-1 blanks before the final one and the
    U labels in all C(T+U-1, U) orders, the final blank at (T-1, U)"""
    T, U = f.shape[0], len(lab)
    p = np.exp(log_probs(f, g[:U + 1]))
    total, count = 0.0, 0
    for emits in itertools.combinations(range(T + U - 1), U):
        t = u = 0
        prob = 1.0
        for step in range(T + U - 1):
            if step in emits:
                prob *= p[t, u, lab[u]]
                u += 1
            else:
                prob *= p[t, u, -1]
                t += 1
        assert (t, u) == (T - 1, U)
        total += prob * p[t, u, -1]
        count += 1
    return -np.log(total), count


def greedy_search(f, enc_len, S, g_fn, steps, dtype=np.float64):
    """The lock-step greedy search, `steps` iterations: row b, while t_pos < enc_len and out_len < S, takes the arg-max
    (smallest index among equal maxima) of f[b,t_pos] + g_fn(b, ids so far); the blank advances t_pos, a label is
    appended.  Returns (ids [B,S] padded with -1, out_len, t_pos, score, margins, paths): margins[b] lists best minus
    second-best joint logit of every decision of row b, paths[b] its (frame, class)."""
    B, T, C = f.shape
    ids = np.full((B, S), -1, np.int32)
    out_len, t_pos = np.zeros(B, np.int32), np.zeros(B, np.int32)
    score = np.zeros(B, dtype)
    margins, paths = [[] for _ in range(B)], [[] for _ in range(B)]
    for b in range(B):
        for _ in range(steps):
            if t_pos[b] >= min(int(enc_len[b]), T) or out_len[b] >= S:
                break
            x = (f[b, t_pos[b]].astype(dtype) + np.asarray(g_fn(b, ids[b, :out_len[b]])).astype(dtype)).astype(dtype)
            k = int(np.argmax(x))                 # (the first of equal maxima)
            top = np.sort(x)
            margins[b].append(float(top[-1] - top[-2]))
            paths[b].append((int(t_pos[b]), k))
            score[b] += (x[k] - x[k]) - np.log(np.exp(x - x[k]).sum(dtype=dtype))
            if k == C - 1:
                t_pos[b] += 1
            else:
                ids[b, out_len[b]] = k
                out_len[b] += 1
    return ids, out_len, t_pos, score, margins, paths
