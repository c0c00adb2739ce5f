"""nabu_ctc_align (csrc/ctc_align.hip) against the float64 restatement of tests/ctc_align_ref.py.

Cases and checks: tests/ctc_align_check.py.  On the quarter grid every partial sum is exact in float32, so state and
seg must equal the reference's element for element — that pins the tie rule, the skip condition on repeated labels and
the end rule.  In this process the default dispatch runs (the wave route for Lmax <= 63); ONE child process runs the
wave-eligible grid cases with NABU_CTC_ALIGN_WORKGROUP=1 and the parent compares bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ctc_align_check as ck
from tests import ctc_align_ref as ar
from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_default = {}          # grid id -> the five outputs of the default dispatch (computed once, read by the forced check)


def _default_run(entry):
    key = ck.grid_id(entry)
    if key not in _default:
        _default[key] = ck.run(*ck.grid_case(*entry))
    return _default[key]


@pytest.mark.parametrize('entry', ck.GRID, ids=[ck.grid_id(e) for e in ck.GRID])
def test_grid_paths_equal_the_reference_exactly(entry):
    """state and seg element for element, the tail of state -1, status 0; score and conf within K_NLL times the
    twin's error plus judge()'s floor of 4 U (ck.scalar_failures, judge_floor); two calls: same bits"""
    assert not ck.forced_workgroup(), 'NABU_CTC_ALIGN_WORKGROUP is set: this test would not reach the wave route'
    case = ck.grid_case(*entry)
    logits, logit_len, labels, label_len = case
    out = _default_run(entry)
    state, seg, conf, score, status = out
    r_state, r_seg, r_conf, r_score, r_status = ar.align(*case)
    assert status == 0 == r_status
    assert state.dtype == np.int32 and seg.dtype == np.int32 and conf.dtype == np.float32 and score.dtype == np.float32
    assert np.array_equal(state, r_state), np.argwhere(state != r_state)[:5]
    assert np.array_equal(seg, r_seg), np.argwhere(seg != r_seg)[:5]
    for b in range(len(logit_len)):
        assert np.all(state[b, logit_len[b]:] == -1)
        assert np.all(conf[b, label_len[b]:] == 0)
    bad, figures = ck.scalar_failures(case, out, judge_floor=True)
    print(ck.grid_id(entry), figures)
    assert not bad, (bad, figures)
    again = ck.run(*case)
    assert again[4] == 0 and ck.same_bits(again[:4], out[:4]), 'second call differs from the first'


def test_workgroup_route_on_the_wave_routes_shapes(tmp_path):
    """the switch is read once per process: a fresh child runs the wave-eligible grid cases on the workgroup route;
    all five outputs must be the default dispatch's, bit for bit"""
    todo = [e for e in ck.GRID if ck.wave_eligible(e[0][1], e[0][3])]
    assert len(todo) >= 8
    path = str(tmp_path / 'forced.npz')
    e = dict(os.environ)
    e['NABU_CTC_ALIGN_WORKGROUP'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'ctc_align_check.py'), path], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'ALIGN DONE' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    with np.load(path) as forced:
        for entry in todo:
            key = ck.grid_id(entry)
            out = _default_run(entry)
            other = [forced['%s/%s' % (key, n)] for n in ('state', 'seg', 'conf', 'score')]
            assert int(forced[key + '/status']) == out[4] == 0, key
            for name, a, c in zip(('state', 'seg', 'conf', 'score'), out[:4], other):
                assert ck.same_bits([a], [c]), '%s: %s differs between the routes' % (key, name)


@pytest.mark.parametrize('entry', ck.CONTINUOUS, ids=['%dx%dx%dx%d-%s' % (s + (r,)) for s, r in ck.CONTINUOUS])
def test_continuous_logits(entry):
    """ctc_cases.make_case logits ('loose' lattices).  The device's path is a valid path that collapses to the labels;
    its float64 raw score is >= the float64 reference's best minus K_NLL times the float32 twin's error on its own
    best path (largest over the utterances of the case) — where that error is exactly 0, the floor 4 U sum|logits
    along the path| is used instead; score and conf: ck.scalar_failures, allowance K_NLL times the twin's error with
    the floor 4 U sum|terms| where the twin's error is exactly 0."""
    shape, regime = entry
    case = ck.continuous_case(shape, regime)
    logits, logit_len, labels, label_len = case
    B, T, C, Lmax = shape
    out = ck.run(*case)
    state, seg, conf, score, status = out
    assert status == 0
    _, _, raw, _, rabs = ar.path_values(logits, logit_len, labels, label_len, state)
    best64, e32 = np.zeros(B), np.zeros(B)
    for b in range(B):
        Tb, lab = int(logit_len[b]), labels[b, :label_len[b]]
        assert not ar.check_path(state[b], Tb, lab, T), (b, ar.check_path(state[b], Tb, lab, T))
        cls = ar.extended(lab, C - 1)[state[b, :Tb]]
        assert ar.collapse(cls, C - 1) == [int(l) for l in lab], b
        assert np.array_equal(seg[b, :len(lab)], ar.segments(state[b, :Tb], len(lab))) and np.all(seg[b, len(lab):] == -1)
        _, best64[b] = ar.viterbi(logits[b, :Tb], lab, np.float64)
        p32, v32 = ar.viterbi(logits[b, :Tb], lab, np.float32)
        x = logits[b, :Tb].astype(np.float64)
        e32[b] = abs(float(v32) - x[np.arange(Tb), ar.extended(lab, C - 1)[p32]].sum())
    tol = cc.K_NLL * e32.max() if e32.max() > 0 else 4 * cc.U * rabs.max()
    print(entry, 'raw gap %.3e, allowance %.3e (twin %.3e)' % ((best64 - raw).max(), tol, e32.max()))
    assert np.all(raw >= best64 - tol), (best64 - raw, tol)
    bad, figures = ck.scalar_failures(case, out)
    print(entry, figures)
    assert not bad, (bad, figures)


def test_invalid_rows_beside_valid_ones():
    """ordinary rejected input: a label = C-1, a row with L + repeats = Tb + 1, two good rows"""
    B, T, C, Lmax = 4, 20, 7, 5
    rng = np.random.default_rng(11)
    logits = ar.grid_logits(rng, (B, T, C))
    labels = rng.integers(0, C - 1, (B, Lmax)).astype(np.int32)
    label_len = np.array([4, 3, 5, 2], np.int32)
    logit_len = np.array([20, 17, 20, 12], np.int32)
    labels[1, 1] = C - 1                                   # row 1: the blank as a label
    labels[2] = [0, 0, 1, 1, 2]
    logit_len[2] = 5 + 2 - 1                               # row 2: one frame short of L + repeats
    state, seg, conf, score, status = ck.run(logits, logit_len, labels, label_len)
    r_state, r_seg, r_conf, r_score, r_status = ar.align(logits, logit_len, labels, label_len)
    assert status == 2 == r_status                         # the first bad row
    for b in (1, 2):
        assert np.isneginf(score[b]) and np.all(state[b] == -1) and np.all(seg[b] == -1) and np.all(conf[b] == 0)
    for b in (0, 3):
        assert np.array_equal(state[b], r_state[b]) and np.array_equal(seg[b], r_seg[b])
        assert np.isfinite(score[b])
    bad, figures = ck.scalar_failures((logits, logit_len, labels, label_len), (state, seg, conf, score, status),
                                      judge_floor=True)
    assert not bad, (bad, figures)         # (the statistic runs over the good rows: the others have no path)
    # one more frame and row 2 is aligned, on its single path
    logit_len[2] += 1
    labels[1, 1] = 0
    state, seg, conf, score, status = ck.run(logits, logit_len, labels, label_len)
    assert status == 0 and state[2, :7].tolist() == [1, 2, 3, 5, 6, 7, 9]
