"""Transducer test cases and their yardstick (plain NumPy; importable without a GPU).

make_case() builds the inputs of one case in the regimes of tests/ctc_cases.py (same sigma, same boost); judge()
compares a result with tests/transducer_ref.py run in float64, allowing a multiple of what THE SAME restatement run in
float32 loses on that case.  The constants are ctc_cases' own, imported: K = 4 for df, dg and their row sums, K_NLL = 16
for the nll.  The reasoning written there carries over: the lattice is a chain of two-term log-sum-exps (the sweeps of
csrc/transducer.hip use the hardware exp2 / log2 at 1 ulp where NumPy's libm is within 0.5 ulp, and scale their
arguments: about twice the roundings of the float32 restatement), the gradient multiplies the errors of two sweeps,
and the nll is ONE number per utterance — the end of a random walk of T_b + U_b roundings at an ulp of |beta| on either
side, whose quotient is half-Cauchy even for a perfect float32 kernel.
Floors: 8 * 2^-24 * max(1, max|g64|) for gradients and row sums, 4 * 2^-24 for the relative nll error."""
import collections

import numpy as np

from tests import transducer_ref as tr
from tests.ctc_cases import BOOST, K, K_NLL, REGIMES, SIGMA, U


class Case(object):
    """f [B,T,C], g [B,U1,C] float32; enc_len, label_len [B], labels [B,Lmax] int32; U1 = Lmax + 1"""

    def __init__(self, f, g, enc_len, labels, label_len, meta):
        self.f, self.g, self.enc_len, self.labels, self.label_len, self.meta = f, g, enc_len, labels, label_len, meta
        self._ref = None

    def __iter__(self):
        return iter((self.f, self.g, self.enc_len, self.labels, self.label_len))

    def reference(self):
        """(n64, df64, dg64, n32, df32, dg32): the restatement in float64 and the same code in float32, computed once"""
        if self._ref is None:
            n64, df64, dg64, st = tr.loss_grad(*self, dtype=np.float64)
            with np.errstate(over='ignore', under='ignore'):
                n32, df32, dg32, _ = tr.loss_grad(*self, dtype=np.float32)
            assert st == 0 and n32.dtype == np.float32 and df32.dtype == np.float32 and dg32.dtype == np.float32
            self._ref = (n64, df64, dg64, n32.astype(np.float64), df32.astype(np.float64), dg32.astype(np.float64))
            for a in self._ref:
                a.setflags(write=False)
        return self._ref


def _path(rng, Tb, Ub):
    """a random valid transducer path as the list of its moves' nodes: Tb blanks and Ub labels, the last move the blank
    at (Tb-1, Ub).  Returns [(t, u, is_label)]"""
    order = np.zeros(Tb + Ub - 1, bool)
    order[rng.permutation(Tb + Ub - 1)[:Ub]] = True
    t = u = 0
    moves = []
    for lab in list(order) + [False]:
        moves.append((t, u, bool(lab)))
        if lab:
            u += 1
        else:
            t += 1
    assert (t, u) == (Tb, Ub)
    return moves


def make_case(B, T, C, Lmax, regime, seed):
    """regime: 'random' N(0, 2) | 'peaky' N(0, 12) | 'aligned' N(0, 2) plus BOOST, added to f, on the class of every
    move of a randomly drawn valid path (the logits of a model that has learnt its alignment: small nll).  Both f and g
    are drawn with the regime's sigma.  Utterance 0 has the full lengths (T, Lmax), the last has label_len = Lmax,
    utterance 1 has label_len = 0 when B >= 3; enc_len is drawn in [max(1, T/2), T].  Labels, lengths and noise depend
    on the seed alone, so the regimes of one seed are comparable."""
    assert regime in REGIMES
    rng = np.random.default_rng(seed)
    label_len = rng.integers(0, Lmax + 1, B)
    labels = rng.integers(0, C - 1, (B, Lmax))
    lo = max(1, T // 2)
    enc_len = lo + np.floor(rng.random(B) * (T - lo + 1)).astype(np.int64)
    nf = rng.standard_normal((B, T, C))
    ng = rng.standard_normal((B, Lmax + 1, C))
    if B >= 3:
        label_len[1] = 0
    label_len[-1] = Lmax
    label_len[0], enc_len[0] = Lmax, T
    f, g = SIGMA[regime] * nf, SIGMA[regime] * ng
    if regime == 'aligned':
        arng = np.random.default_rng([seed, 1])
        for b in range(B):
            for t, u, is_label in _path(arng, int(enc_len[b]), int(label_len[b])):
                f[b, t, labels[b, u] if is_label else C - 1] += BOOST
    meta = dict(B=B, T=T, C=C, Lmax=Lmax, regime=regime, seed=seed)
    return Case(np.ascontiguousarray(f, np.float32), np.ascontiguousarray(g, np.float32), enc_len.astype(np.int32),
                labels.astype(np.int32), label_len.astype(np.int32), meta)


def seed_of(B, T, C, Lmax):
    return 100000 * B + 100 * T + 7 * C + 13 * Lmax


Verdict = collections.namedtuple('Verdict', 'ok report e_ref e_ker s_ref s_ker n_ref n_ker')


def _ratio(ker, ref):
    return ker / ref if ref > 0 else (0.0 if ker == 0 else float('inf'))


def _max(a):
    return float(a.max()) if a.size and np.all(np.isfinite(a)) else (0.0 if not a.size else float('inf'))


def judge(nll, df, dg, case, grad_scale=1.0, k=K, k_nll=K_NLL):
    """Compare (nll [B], df [B,T,C], dg [B,U1,C]) = grad_scale * gradients with the float64 restatement, allowing k
    times what the float32 restatement loses on this case (maxima over df and dg together):
      gradient  e_ker = max|d/grad_scale - g64|                      <= k * max|g32 - g64| + floor
      row sums  s_ker = max over rows inside the lengths |sum_k d|   <= k * the same of g32 + floor   (exactly 0 in g64)
      nll       n_ker = max_b |nll - n64| / |n64|                    <= k_nll * max_b |n32 - n64| / |n64| + 4 * 2^-24
    with floor = 8 * 2^-24 * max(1, max|g64|)."""
    n64, df64, dg64, n32, df32, dg32 = case.reference()
    nll = np.asarray(nll, np.float64)
    df, dg = np.asarray(df, np.float64) / grad_scale, np.asarray(dg, np.float64) / grad_scale
    assert nll.shape == n64.shape and df.shape == df64.shape and dg.shape == dg64.shape, (nll.shape, df.shape, dg.shape)
    floor = 8 * U * max(1.0, float(np.abs(df64).max()), float(np.abs(dg64).max()))
    msgs = []
    e_ref = max(_max(np.abs(df32 - df64)), _max(np.abs(dg32 - dg64)))
    e_ker = max(_max(np.abs(df - df64)), _max(np.abs(dg - dg64)))
    if not e_ker <= k * e_ref + floor:
        msgs.append('gradient: e_ker %.3e > %g * e_ref %.3e + %.3e (df %.3e, dg %.3e)'
                    % (e_ker, k, e_ref, floor, _max(np.abs(df - df64)), _max(np.abs(dg - dg64))))
    vt = np.arange(df.shape[1])[None, :] < np.asarray(case.enc_len)[:, None]
    vu = np.arange(dg.shape[1])[None, :] <= np.asarray(case.label_len)[:, None]

    def sums(a, b):
        return max(_max(np.abs(np.where(vt, a.sum(2), 0))), _max(np.abs(np.where(vu, b.sum(2), 0))))
    s_ref, s_ker = sums(df32, dg32), sums(df, dg)
    if not s_ker <= k * s_ref + floor:
        msgs.append('row sums: s_ker %.3e > %g * s_ref %.3e + %.3e' % (s_ker, k, s_ref, floor))
    n_ref = _max(np.abs(n32 - n64) / np.abs(n64))
    n_ker = _max(np.abs(nll - n64) / np.abs(n64))
    if not n_ker <= k_nll * n_ref + 4 * U:
        r = np.abs(nll - n64) / np.abs(n64)
        b = int(np.argmax(np.where(np.isfinite(r), r, np.inf)))
        msgs.append('nll: n_ker %.3e > %g * n_ref %.3e + 4u at [b %d]: %.9g, reference %.9g'
                    % (n_ker, k_nll, n_ref, b, nll[b], n64[b]))
    return Verdict(not msgs, '; '.join(msgs), e_ref, e_ker, s_ref, s_ker, n_ref, n_ker)


def needed(v, case):
    """the smallest allowances with which judge() accepts the result: (error - floor) / reference error, >= 0"""
    _, df64, dg64 = case.reference()[:3]
    floor = 8 * U * max(1.0, float(np.abs(df64).max()), float(np.abs(dg64).max()))
    return (_ratio(max(v.e_ker - floor, 0.0), v.e_ref), _ratio(max(v.s_ker - floor, 0.0), v.s_ref),
            _ratio(max(v.n_ker - 4 * U, 0.0), v.n_ref))


# the shapes (B, T, C, Lmax) of tests/test_hip_transducer.py, by group
SHAPES = [
    ('small', [(1, 1, 2, 0), (2, 1, 3, 2), (3, 2, 3, 1)]),
    ('lanes', [(4, 70, 40, 62), (4, 70, 40, 63), (4, 70, 40, 64)]),        # lane 63; Lmax = 64: the workgroup route
    ('stride', [(2, 40, 12, 255), (2, 40, 12, 256)]),                      # u strided over 256 threads
    ('classes', [(3, 12, 64, 6), (3, 12, 65, 6), (3, 12, 193, 6), (3, 12, 257, 6)]),
    ('corners', [(3, 300, 40, 5), (3, 4, 40, 60)]),                        # the diagonals' clamps at both ends
]
ALL_SHAPES = [s for _, group in SHAPES for s in group]


def wave_eligible(Lmax):
    """the dispatch of nabu_transducer_loss_grad without the switch: one wave64 per sweep and utterance"""
    return Lmax + 1 <= 64


def shift_case(case, seed):
    """(shifted case, unshifted case): `case` with f and g rounded to multiples of 2^-10, and the same with a constant
    of +80 or -80 added to every row of f and of g.  On that grid, with |x| < 2^13, the shifted rows and every joint
    logit f + g are exact in float32, so the shifted problem IS the unshifted one plus a constant per node: a kernel
    that subtracts each node's own maximum loses nothing, one that carries the constants into exp or keeps max + log-sum
    as one number does."""
    q = 2.0 ** -10
    f0 = (np.round(case.f.astype(np.float64) / q) * q).astype(np.float32)
    g0 = (np.round(case.g.astype(np.float64) / q) * q).astype(np.float32)
    rng = np.random.default_rng([seed, 2])
    cf = rng.choice([80.0, -80.0], size=f0.shape[:2]).astype(np.float32)
    cg = rng.choice([80.0, -80.0], size=g0.shape[:2]).astype(np.float32)
    f1, g1 = f0 + cf[:, :, None], g0 + cg[:, :, None]
    assert np.array_equal(f1.astype(np.float64), f0.astype(np.float64) + cf[:, :, None]), 'the shift of f is not exact'
    assert np.array_equal(g1.astype(np.float64), g0.astype(np.float64) + cg[:, :, None]), 'the shift of g is not exact'
    plain = Case(f0, g0, case.enc_len, case.labels, case.label_len, dict(case.meta, shift=0))
    moved = Case(f1, g1, case.enc_len, case.labels, case.label_len, dict(case.meta, shift=80))
    return moved, plain
