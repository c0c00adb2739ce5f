"""CPU tests of the transducer yardstick (tests/transducer_ref.py, tests/transducer_cases.py) and of the host-side
contract of nabu_transducer_loss_grad / nabu_transducer_greedy_step: the restatement against an enumeration of every
path and against central differences, its row sums and zero rows, the case generator's promises, judge() on itself."""
import ctypes
import math

import numpy as np
import pytest

from tests import ctc_cases as cc
from tests import transducer_cases as tc
from tests import transducer_ref as tr

ENUM = [(1, 0, 2), (1, 2, 3), (3, 2, 4), (4, 3, 5), (5, 0, 3)]          # (T, U, C)


def _one(T, U, C, seed=0, sigma=2.0):
    rng = np.random.default_rng([seed, T, U, C])
    f = sigma * rng.standard_normal((1, T, C))
    g = sigma * rng.standard_normal((1, U + 1, C))
    labels = rng.integers(0, C - 1, (1, max(U, 1))).astype(np.int32)
    return f, g, np.array([T], np.int32), labels, np.array([U], np.int32)


@pytest.mark.parametrize('T,U,C', ENUM)
def test_nll_is_the_sum_over_every_path(T, U, C):
    f, g, enc_len, labels, label_len = _one(T, U, C)
    nll, _, _, status = tr.loss_grad(f, g, enc_len, labels, label_len)
    brute, count = tr.brute_force_nll(f[0], g[0], labels[0, :U])
    assert status == 0 and count == math.comb(T + U - 1, U)
    assert abs(nll[0] - brute) <= 1e-12 * max(1.0, abs(brute)), (nll[0], brute)
    # alpha reaches the same number from the other end
    lp = tr.log_probs(f[0], g[0])
    lb, _, alpha, beta = tr.lattice(lp, labels[0, :U])
    assert abs((alpha[T - 1, U] + lb[T - 1, U]) - beta[0, 0]) <= 1e-12 * max(1.0, abs(brute))


@pytest.mark.parametrize('T,U,C', ENUM)
def test_gradients_are_the_central_differences(T, U, C):
    f, g, enc_len, labels, label_len = _one(T, U, C, seed=1)
    _, df, dg, _ = tr.loss_grad(f, g, enc_len, labels, label_len)
    eps = 1e-6
    for arr, grad in ((f, df), (g, dg)):
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + eps
            up = tr.loss_grad(f, g, enc_len, labels, label_len)[0][0]
            arr[idx] = keep - eps
            dn = tr.loss_grad(f, g, enc_len, labels, label_len)[0][0]
            arr[idx] = keep
            assert abs((up - dn) / (2 * eps) - grad[idx]) <= 1e-8, (idx, (up - dn) / (2 * eps), grad[idx])


def test_row_sums_zero_rows_and_the_float32_run():
    case = tc.make_case(4, 9, 6, 4, 'random', 3)
    n64, df64, dg64, n32, df32, dg32 = case.reference()
    for b in range(4):
        Tb, Ub = int(case.enc_len[b]), int(case.label_len[b])
        assert np.abs(df64[b, :Tb].sum(1)).max() <= 1e-14 and np.abs(dg64[b, :Ub + 1].sum(1)).max() <= 1e-14
        assert np.all(df64[b, Tb:] == 0) and np.all(dg64[b, Ub + 1:] == 0)
        assert np.all(df32[b, Tb:] == 0) and np.all(dg32[b, Ub + 1:] == 0)
    assert 0 < np.abs(df32 - df64).max() < 1e-5 and 0 < np.abs(n32 - n64).max() < 1e-4 * np.abs(n64).max()
    assert np.abs(df64.sum(1) + 0).max() > 0       # (not a vacuous case)


def test_invalid_utterances_of_the_reference():
    f, g = np.zeros((4, 3, 4)), np.zeros((4, 3, 4))
    labels = np.array([[0, 1], [3, 0], [1, 1], [0, -1]], np.int32)
    nll, df, dg, status = tr.loss_grad(f, g, np.array([3, 3, 4, 3]), labels, np.array([2, 2, 2, 1]))
    assert status == 2 and nll[1] == 0 and nll[2] == 0 and nll[0] > 0 and nll[3] > 0     # (row 3's -1 lies past its length)
    assert np.all(df[1:3] == 0) and np.all(dg[1:3] == 0) and np.any(df[0] != 0)
    assert tr.loss_grad(f, g, np.array([3, 3, 0, 3]), labels, np.array([2, 0, 3, -1]))[3] == 3


def test_make_case_promises():
    for shape in [(1, 1, 2, 0), (3, 2, 3, 1), (4, 20, 7, 5)]:
        B, T, C, Lmax = shape
        cases = [tc.make_case(B, T, C, Lmax, r, tc.seed_of(*shape)) for r in cc.REGIMES]
        for c in cases:
            assert c.f.shape == (B, T, C) and c.g.shape == (B, Lmax + 1, C) and c.f.dtype == np.float32
            assert c.enc_len[0] == T and c.label_len[0] == Lmax and c.label_len[-1] == Lmax
            assert np.all((c.enc_len >= 1) & (c.enc_len <= T)) and np.all((c.label_len >= 0) & (c.label_len <= Lmax))
            assert B < 3 or c.label_len[1] == 0
            assert np.all((c.labels >= 0) & (c.labels < C - 1)) if Lmax else c.labels.size == 0
            assert np.array_equal(c.labels, cases[0].labels) and np.array_equal(c.enc_len, cases[0].enc_len)
        if shape[1] > 2:
            n = [c.reference()[0].mean() for c in cases]
            assert n[2] < n[0] < n[1], n              # aligned < random < peaky
    assert (tc.K, tc.K_NLL, tc.U) == (cc.K, cc.K_NLL, cc.U) == (4.0, 16.0, 2.0 ** -24)
    assert tc.SIGMA is cc.SIGMA and tc.BOOST == cc.BOOST


def test_judge_accepts_the_float32_run_and_rejects_a_perturbed_one():
    case = tc.make_case(3, 12, 8, 4, 'random', 5)
    n64, df64, dg64, n32, df32, dg32 = case.reference()
    v = tc.judge(n32, df32, dg32, case)
    assert v.ok and v.e_ker == v.e_ref and tc.needed(v, case)[0] <= 1.0
    assert tc.judge(n32, 0.25 * df32, 0.25 * dg32, case, grad_scale=0.25).ok
    bad = df32.copy()
    bad[0, 0, 0] += 1e-4
    v = tc.judge(n32, bad, dg32, case)
    assert not v.ok and 'gradient' in v.report and 'row sums' in v.report
    assert not tc.judge(n32 * (1 + 1e-4), df32, dg32, case).ok
    nan = df32.copy()
    nan[1, 1, 1] = np.nan
    assert not tc.judge(n32, nan, dg32, case).ok


def test_shift_case_is_exact():
    case = tc.make_case(3, 12, 8, 4, 'peaky', 5)
    moved, plain = tc.shift_case(case, 5)
    h1 = moved.f[:, :, None, :] + moved.g[:, None, :, :]                       # float32
    h0 = plain.f[:, :, None, :].astype(np.float64) + plain.g[:, None, :, :].astype(np.float64)
    shift = (moved.f[:, :, 0] - plain.f[:, :, 0])[:, :, None] + (moved.g[:, :, 0] - plain.g[:, :, 0])[:, None, :]
    assert h1.dtype == np.float32 and np.array_equal(h1.astype(np.float64), h0 + shift[..., None])
    assert set(np.unique(shift)) <= {-160.0, 0.0, 160.0} and len(np.unique(shift)) == 3
    a, b = moved.reference(), plain.reference()
    assert np.abs(a[0] - b[0]).max() <= 1e-9 and np.abs(a[1] - b[1]).max() <= 1e-12


def test_greedy_search_of_the_reference():
    C, S = 4, 3
    f = np.zeros((2, 3, C))
    f[0, 0, 1] = 2.0         # frame 0: label 1, then (history 1) label 2, then the blank
    f[0, 1, 3] = 1.0
    f[0, 2, 3] = 1.0
    f[1, :, 0] = 1.0         # row 1 emits label 0 until it reaches S

    def g_fn(b, ids):
        g = np.zeros(C)
        if b == 0 and len(ids) == 1:
            g[2] = 3.0
        if b == 0 and len(ids) == 2:
            g[3] = 3.0
        return g
    ids, out_len, t_pos, score, margins, paths = tr.greedy_search(f, np.array([3, 2]), S, g_fn, 10)
    assert ids.tolist() == [[1, 2, -1], [0, 0, 0]] and out_len.tolist() == [2, 3] and t_pos.tolist() == [3, 0]
    assert len(margins[0]) == 5 and len(margins[1]) == 3 and np.all(score < 0)
    assert paths[0] == [(0, 1), (0, 2), (0, 3), (1, 3), (2, 3)] and paths[1] == [(0, 0)] * 3
    # equal maxima: the smallest index
    tie = np.zeros((1, 1, C))
    assert tr.greedy_search(tie, np.array([1]), 2, lambda b, ids: np.zeros(C), 5)[0].tolist() == [[0, 0]]


def test_host_side_contract_of_the_transducer_entry_points():
    """size query and argument validation: all on the host, before any launch (no GPU needed)"""
    from nabu_amd import build, _hip
    build.build(verbose=False)
    lib = _hip.lib()
    ws = lib.nabu_transducer_ws_bytes
    for shape in ((0, 10, 3), (-1, 10, 3), (4, 0, 3), (4, 10, 0), (4, 10, -1)):
        assert ws(*shape) == 0, shape
    assert ws(2, 10, 4) >= 5 * 2 * 10 * 4 * 4          # Z, lb, ly, alpha, beta of every node at least
    one = ctypes.c_void_p(16)        # any non-null pointer: validation happens before it is touched
    big = 1 << 40

    def call(B=2, T=5, U1=4, C=4, f=one, g=one, el=one, lab=one, ldl=3, ll=one, nll=one, df=one, dg=one, status=one,
             w=one, wb=big):
        return lib.nabu_transducer_loss_grad(B, T, U1, C, f, g, el, lab, ldl, ll, 1.0, nll, df, dg, status, w, wb, None)

    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(U1=0), dict(C=1), dict(f=None), dict(g=None), dict(el=None),
               dict(ll=None), dict(nll=None), dict(df=None), dict(dg=None), dict(status=None), dict(w=None), dict(ldl=2),
               dict(lab=None)):
        assert call(**kw) == -1, kw
    assert b'labels' in lib.nabu_last_error()
    assert call(wb=ws(2, 5, 4) - 1) == -3 and b'workspace' in lib.nabu_last_error()

    def step(B=2, T=5, C=4, S=3, step=0, ptrs=(one,) * 9):
        return lib.nabu_transducer_greedy_step(B, T, C, S, step, *(ptrs + (None,)))
    for kw in (dict(B=0), dict(T=0), dict(C=1), dict(S=0), dict(step=-1)):
        assert step(**kw) == -1, kw
    for i in range(9):
        assert step(ptrs=(one,) * i + (None,) + (one,) * (8 - i)) == -1, i
    assert b'null pointer' in lib.nabu_last_error()
