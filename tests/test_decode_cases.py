"""CPU tests of the CTC beam-search case tables (tests/decode_cases.py): every committed seed still meets, on the
float64 oracle alone, the conditions that tests/test_hip_decode_limits.py asserts before it touches the device, and
the yardstick itself refuses what it should."""
import numpy as np
import pytest

from oracle import decode_oracle as D
from tests import decode_cases as dc


@pytest.mark.parametrize('W,C,T,seeds', dc.WIDTH_CASES, ids=['W%d' % c[0] for c in dc.WIDTH_CASES])
def test_width_cases_decide_at_w_and_are_admissible(W, C, T, seeds):
    assert T <= 6 and C == (5 if W <= 8 else 40) and len(seeds) <= 4
    logits = dc.width_case(W, C, T, seeds)
    assert logits.dtype == np.float32 and logits.shape == (len(seeds), T, C)
    # early frames flat, late frames peaked
    spread = logits.max(2) - logits.min(2)
    assert spread[:, :2].max() < 1.0 < spread[:, -2:].min()
    for seed, x in zip(seeds, logits):
        det, below, above = dc.width_decides(x, W)
        assert det['labels'] != above and (W == 1 or det['labels'] != below), seed
        assert dc.inadmissible(det, T) is None, (seed, dc.inadmissible(det, T))
        assert dc.width_ok(x, W), seed


def test_width_cases_cover_the_widths_of_the_issue():
    assert [c[0] for c in dc.WIDTH_CASES] == [1, 2, 8, 100, 256]


@pytest.mark.parametrize('name', sorted(dc.PLAIN_CASES))
def test_plain_cases_are_admissible(name):
    logits, lens, W, merges = dc.plain_case(name, dc.PLAIN_CASES[name])
    assert logits.shape[0] <= 4 and dc.all_admissible(logits, lens, W, merges)
    dets = dc.oracle(logits, lens, W)
    assert all(d['select_ties'] == 0 for d in dets)
    if name == 'max_width':
        assert W == 256 and len(dets[0]['beam']) == 256 and np.isfinite(dets[0]['select_gap'])
    if name == 'one_label':
        assert logits.shape[1:] == (9, 2) and W == 4 and merges == (True, False)
    if name == 'lengths':
        T = logits.shape[1]
        assert list(lens) == [1, T, T + 5]
        assert dets[2]['labels'] == D.ctc_beam_search(logits[2], W)
    if name == 'neg_inf':
        assert np.isneginf(logits[0]).any(0)[:4].any() and np.isfinite(logits[0, :, 4]).all()
        assert np.isneginf(logits[1, 2, :4]).all() and np.isfinite(logits[1, 2, 4])
        assert np.isneginf(logits[2, 3, 4]) and np.isfinite(logits[2, 3, :4]).all()
        assert dets[3]['labels'] == [] and dets[3]['total'] == -np.inf and dets[3]['beam'] == []
        assert all(d['labels'] and np.isfinite(d['total']) for d in dets[:3])


def test_tie_case_cuts_through_a_tied_group():
    C, T, W, seeds = dc.TIE_CASE
    for seed in seeds:
        x = dc.tie_logits(C, T, seed)
        assert np.array_equal(x[:, dc.TIE_A], x[:, dc.TIE_B]) and np.ptp(x) > 1       # not uniform
        assert dc.tie_ok(x, W), seed
        for merge in (True, False):
            det = D.ctc_beam_search(x, W, merge, details=True)
            assert det['select_ties'] > 0 and dc.inadmissible(det, T, ties=True) is None
            assert dc.inadmissible(det, T) is not None                              # ties are refused unless built


def test_yardstick_refuses_narrow_margins():
    det = dict(select_gap=1e-3, top_gap=1e-3, order_gap=1e-3, select_ties=0, max_abs_total=10.0)
    g = dc.guard_bound(6, det)
    assert g == 4 * 6 * 2.0 ** -23 * 10.0 and dc.lp_bound(6, -10.0) == g / 2 and dc.lp_bound(6, -0.5) == g / 20
    assert dc.inadmissible(det, 6) is None
    for key in ('select_gap', 'top_gap'):
        assert key in dc.inadmissible(dict(det, **{key: g}), 6)
    assert 'ties' in dc.inadmissible(dict(det, select_ties=1), 6)
    assert dc.inadmissible(dict(det, select_ties=1), 6, ties=True) is None
    assert 'order_gap' in dc.inadmissible(dict(det, select_ties=1, order_gap=g), 6, ties=True)
    assert dc.inadmissible(dict(det, order_gap=0.0), 6) is None
