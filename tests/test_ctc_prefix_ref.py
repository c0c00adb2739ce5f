"""tests/ctc_prefix_ref.py held to an enumeration of all paths (CPU): the recurrences of the CTC prefix score that
the GPU tests (tests/test_hip_ctc_prefix.py) measure the kernels against."""
import itertools

import numpy as np
import pytest

from tests import ctc_prefix_ref as R


def _y(T, C, seed, sigma=1.0):
    rng = np.random.default_rng(seed)
    return R.log_softmax(sigma * rng.standard_normal((T, C)))[0]


@pytest.mark.parametrize('T,C', [(5, 3), (6, 4)])
def test_prefix_scores_equal_the_sum_over_all_paths(T, C):
    y = _y(T, C, 10 * T + C)
    table = R.enumerate_prefixes(y, 3)
    assert len(table) == sum((C - 1) ** n for n in range(4))
    worst = 0.0
    for g, (start, exact) in table.items():
        st, psi, last = R.prefix_state(y, T, g)
        end = R.psi_all(y, T, st, last)[C - 1]
        for got, want in ((psi, start), (end, exact)):
            if want == -np.inf:
                assert got <= -1e29, (g, got)
            else:
                worst = max(worst, abs(got - want))
    assert worst < 1e-13, worst


@pytest.mark.parametrize('T,C', [(5, 3), (6, 4)])
def test_extensions_and_the_end_label_partition_the_prefix(T, C):
    """sum_c exp psi(g.c) + exp psi(g.eos) = exp psi(g)"""
    y = _y(T, C, 7 * T + C, sigma=2.0)
    for n in range(4):
        for g in itertools.product(range(C - 1), repeat=n):
            st, psi, last = R.prefix_state(y, T, g)
            if psi <= -1e29:
                continue
            parts = R.psi_all(y, T, st, last)
            assert np.exp(parts).sum() == pytest.approx(np.exp(psi), rel=1e-12), g


def test_shorter_utterance_inside_a_longer_array():
    """frames beyond the length are not part of the utterance"""
    y = _y(6, 4, 3)
    table = R.enumerate_prefixes(y[:4], 2)
    for g, (start, exact) in table.items():
        st, psi, last = R.prefix_state(y, 4, g)
        if start > -np.inf:
            assert psi == pytest.approx(start, abs=1e-13)
        if exact > -np.inf:
            assert R.psi_all(y, 4, st, last)[3] == pytest.approx(exact, abs=1e-13)
        assert np.all(st[4:] == R.NEG)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_infeasible_prefixes_score_log_zero_and_stay_there(dtype):
    y = R.log_softmax(np.random.default_rng(5).standard_normal((3, 4)), dtype)[0]
    assert y.dtype == dtype
    for g, Tb in (((0, 1, 2, 0), 3),       # longer than the utterance
                  ((1, 1), 2),             # the repeat needs a blank that two frames do not leave
                  ((0,), 0)):              # no frames at all
        st, psi, last = R.prefix_state(y, Tb, g)
        assert psi == dtype(R.NEG) and st.dtype == dtype
        parts = R.psi_all(y, Tb, st, last)
        assert parts.dtype == dtype and np.all(parts == dtype(R.NEG)), (g, parts)      # every extension, and eos
        assert np.all(parts - psi == 0)                                                # delta: 0, not NaN
        st2, psi2 = R.extend(y, Tb, st, last, 2)
        assert psi2 == dtype(R.NEG) and np.all(np.isfinite(st2))
    # feasible, but only just: one path
    st, psi, last = R.prefix_state(y, 3, (1, 1))
    assert psi == pytest.approx(y[0, 1] + y[1, 3] + y[2, 1], rel=1e-6)


def test_batch_functions_agree_with_the_single_hypothesis_ones():
    rng = np.random.default_rng(11)
    B, W, T, C = 2, 3, 6, 4
    logits = rng.standard_normal((B, T, C)).astype(np.float32)
    enc_len = np.array([6, 4], np.int32)
    y, beam = R.prepare(logits, enc_len, W)
    assert np.all(beam['psi'] == 0) and np.all(beam['last'] == -1)
    parent = np.array([[0, 0, 1], [2, 2, 0]], np.int32)
    pred = np.array([[1, 2, 3], [0, 3, 0]], np.int32)
    stay = np.zeros((B, W), np.int32)
    one = R.advance(y, enc_len, beam, parent, stay, pred)
    fin = (pred == C - 1).astype(np.int32)
    parent2 = np.array([[0, 1, 2], [1, 0, 2]], np.int32)
    pred2 = np.array([[1, 0, 3], [3, 0, 1]], np.int32)
    stay2 = np.array([[0, 0, 1], [1, 0, 0]], np.int32)
    two = R.advance(y, enc_len, one, parent2, stay2, pred2)
    hyps = {(0, 0): (1, 1), (0, 1): (2, 0), (0, 2): (), (1, 0): (), (1, 1): (0, 0), (1, 2): (0, 1)}
    for (b, k), g in hyps.items():
        st, psi, last = R.prefix_state(y[b], int(enc_len[b]), g)
        assert np.array_equal(two['state'][b, k], st) and two['last'][b, k] == last, (b, k)
        if (b, k) in ((0, 2), (1, 0)):          # finished with eos: psi is that of the exact labelling
            assert two['psi'][b, k] == R.psi_all(y[b], int(enc_len[b]), st, last)[C - 1]
        else:
            assert two['psi'][b, k] == psi
    d = R.score(y, enc_len, one, fin)
    assert np.all(d[0, 2] == 0) and np.all(d[1, 1] == 0) and np.all(d[0, 0, :C - 1] < 0)
