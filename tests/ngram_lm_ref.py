"""The label n-gram of nabu_amd/processing/ngram_lm.py restated on dictionaries of tuples (plain Python / NumPy float64;
importable without a GPU).  Nothing here imports the module under test.

Symbols 0..C-2 are labels, C-1 is the boundary.  A sentence is padded with n-1 boundaries in front and one at the end;
count_k(h, c), h a tuple of k-1 symbols (oldest first), counts the positions — every label and the final boundary —
preceded by h and holding c.  Interpolated Witten-Bell:
    p_k(c|h) = (count(h,c) + N1+(h) p_{k-1}(c|h[1:])) / (count(h) + N1+(h)),  p_k(c|h) = p_{k-1}(c|h[1:]) if count(h) = 0,
    p_0 = 1/C."""
import itertools
from collections import defaultdict

import numpy as np


def counts(sentences, C, n):
    """[k-1] -> {h tuple of k-1 symbols: {c: count}} for k = 1..n"""
    out = [defaultdict(lambda: defaultdict(int)) for _ in range(n)]
    for s in sentences:
        padded = [C - 1] * (n - 1) + [int(x) for x in s] + [C - 1]
        for i in range(n - 1, len(padded)):
            for k in range(1, n + 1):
                out[k - 1][tuple(padded[i - k + 1:i])][padded[i]] += 1
    return out


def prob(cnt, C, h, c):
    """p_k(c | h) for k = len(h) + 1"""
    if len(h) == 0:
        lower = 1.0 / C
    else:
        lower = prob(cnt, C, h[1:], c)
    succ = cnt[len(h)].get(tuple(h))
    if not succ:
        return lower
    total, n1 = sum(succ.values()), len(succ)
    return (succ.get(c, 0) + n1 * lower) / (total + n1)


def context_index(h, C):
    """a tuple of symbols, oldest first, as the base-C number with the most recent symbol least significant"""
    idx = 0
    for s in h:
        idx = idx * C + int(s)
    return idx


def next_context(ctx, c, C, n):
    return (ctx * C + c) % (C ** (n - 1))


def start_context(C, n):
    return context_index((C - 1,) * (n - 1), C)


def table(sentences, C, n):
    """probabilities [C^(n-1), C] float64"""
    cnt = counts(sentences, C, n)
    p = np.zeros((C ** (n - 1), C))
    for h in itertools.product(range(C), repeat=n - 1):
        for c in range(C):
            p[context_index(h, C), c] = prob(cnt, C, h, c)
    return p


def sequence_logprob(logp, labels, C, n, end=True):
    """log p(labels [. end]) under a table of log-probabilities"""
    ctx, total = start_context(C, n), 0.0
    for c in list(labels) + ([C - 1] if end else []):
        total += float(logp[ctx, c])
        ctx = next_context(ctx, c, C, n)
    return total


def random_table(C, n, seed, sharp=1.5):
    """a seeded table of log-probabilities float32 [C^(n-1), C] (rows normalised in float64, then rounded): what the
    search tests feed both the device and the float64 references"""
    rng = np.random.default_rng([seed, C, n, 77])
    x = sharp * rng.standard_normal((C ** (n - 1), C))
    x = x - x.max(1, keepdims=True)
    x = x - np.log(np.exp(x).sum(1, keepdims=True))
    return x.astype(np.float32)
