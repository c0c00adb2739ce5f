"""CPU tests of the CTC case table and its yardstick (tests/ctc_cases.py) and of the checks the GPU tests apply
(tests/ctc_kernel_check.py): the reference alone stays inside every condition the GPU tests impose, and every one of
those conditions is seen to fail on a deliberately wrong CPU stand-in of the kernel."""
import os

import numpy as np
import pytest

from oracle import nabu_oracle as O
from tests import ctc_cases as cc
from tests import ctc_kernel_check as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [e['id'] for e in cc.CASES]


def test_lds_formula_is_the_one_in_the_source():
    """which kernel a shape reaches is decided in csrc/ctc.hip; ctc_cases restates it — hold the two together"""
    src = open(os.path.join(ROOT, 'nabu_amd', 'csrc', 'ctc.hip')).read()
    for text in (cc.WAVE_LDS_FORMULA, cc.WAVE_DISPATCH, cc.WAVE_LAUNCH):
        assert text in src, text
    # the launch helper raises the attribute above 64 KiB and not below
    helper = open(os.path.join(ROOT, 'nabu_amd', 'csrc', 'common.hip')).read()
    assert cc.WAVE_ATTR in helper and 'hipFuncSetAttribute' not in src
    raise_at, set_at = helper.index(cc.WAVE_ATTR), helper.index('hipFuncSetAttribute(')
    assert helper.count('hipFuncSetAttribute(') == 1 and raise_at < set_at < helper.index('\n  }\n', raise_at)
    assert (cc.T64, cc.T150) == (98, 235)
    assert cc.wave_lds_bytes(cc.T64, 40, 60) <= 64 * 1024 < cc.wave_lds_bytes(cc.T64 + 1, 40, 60)
    assert cc.wave_lds_bytes(cc.T150, 40, 60) <= 150 * 1024 < cc.wave_lds_bytes(cc.T150 + 1, 40, 60)


def test_table_reaches_both_kernels_where_the_issue_wants_them():
    shapes = sorted(set(e['shape'] for e in cc.CASES))
    wave = [s for s in shapes if cc.wave_eligible(*s[1:])]
    once = [s for s in shapes if not cc.wave_eligible(*s[1:])]
    # the shapes that run once, on the workgroup kernel: Lmax >= 64, T just over the 150 KiB limit, cfg1
    assert once == sorted([(4, 140, 40, 64), (3, 300, 40, 127), (3, 300, 40, 128), (3, 236, 40, 60), (8, 1000, 40, 60)])
    assert (4, 140, 40, 63) in wave and (32, 125, 40, 60) in wave and (3, 24, 300, 8) in wave and (1, 1, 2, 0) in wave
    assert len(cc.CASES) == 18 * 6 + 6 + 2 + 2 and len(set(IDS)) == len(IDS)
    # every group with a wave-eligible shape gets its child process
    assert cc.GROUPS == ['classes', 'full', 'lanes', 'lds', 'odd', 'scale', 'small']
    assert cc.K == 4 and cc.K_NLL == 16             # never above 16


@pytest.mark.parametrize('entry', cc.CASES, ids=IDS)
def test_case_is_well_formed_and_the_reference_meets_the_gpu_conditions(entry):
    case = cc.build(entry)
    B, T, C, Lmax = entry['shape']
    logits, tl, labels, ll = case
    assert logits.dtype == np.float32 and logits.shape == (B, T, C) and labels.shape == (B, Lmax)
    assert tl.dtype == ll.dtype == labels.dtype == np.int32
    assert np.all(case.need <= T) and np.all(case.need == cc.needed_frames(labels, ll))
    assert tl[0] == T and ll[-1] == Lmax and np.all((ll >= 0) & (ll <= Lmax)) and np.all((tl >= case.need) & (tl <= T))
    if Lmax >= 2:
        assert ll[0] >= 2 and labels[0, 0] == labels[0, 1]
    if B >= 3:
        assert ll[1] == 0
    if entry['lattice'] == 'tight':
        assert np.all(tl[1:] == case.need[1:])             # utterance 0 keeps the full length
    else:
        assert np.all(tl >= min(T, T // 2))
    n64, g64, n32, g32 = case.oracle()                       # raises on 'Not enough time'
    for a in (n64, g64, n32, g32):
        assert np.all(np.isfinite(a))
    assert np.all(n64 > 0)
    valid = np.arange(T)[None, :] < tl[:, None]
    assert np.abs(np.where(valid, g64.sum(2), 0)).max() < 1e-9     # the identity the frame-sum rule relies on
    assert np.all(g64[~valid] == 0)
    # the float64 oracle passes its own judgement with nothing to spare asked of it, at any grad_scale
    v = cc.judge(n64, g64 * entry['grad_scale'], case, entry['grad_scale'])
    assert v.ok and v.e_ker < 1e-15 and v.n_ker == 0, v.report
    # ... and so does the float32 one (ratio 1 by construction)
    assert cc.judge(n32, g32, case).ok


@pytest.mark.parametrize('shape', sorted(set(e['shape'] for e in cc.CASES)))
def test_aligned_logits_have_the_smaller_nll(shape):
    seed = cc.seed_of(*shape)
    for lattice in cc.LATTICES:
        r = cc.make_case(*shape, regime='random', lattice=lattice, seed=seed)
        a = cc.make_case(*shape, regime='aligned', lattice=lattice, seed=seed)
        assert np.array_equal(r.labels, a.labels) and np.array_equal(r.logit_len, a.logit_len)
        assert np.all(a.oracle()[0] < r.oracle()[0])


# --------------------------------------------------------------------------------------------------------------
# every assertion of the GPU tests, seen to fail once on a wrong CPU stand-in
def _case(shape=(4, 40, 64, 10), regime='aligned', lattice='loose'):
    return cc.make_case(*shape, regime=regime, lattice=lattice, seed=cc.seed_of(*shape))


def test_judge_notices_a_dropped_occupation_of_1e_4():
    case = _case()
    n64, g64, _, _ = case.oracle()
    assert cc.judge(n64, g64, case).ok
    g = g64.copy()
    g[1, 3, case.logits.shape[2] - 1] += 1e-4                 # a blank occupation of 1e-4 never subtracted
    v = cc.judge(n64, g, case)
    assert not v.ok and 'gradient' in v.report and 'frame sums' in v.report and '[b 1, t 3' in v.report
    # it is the well-aligned logits that make this visible: float32 itself loses K * e_ref < 1e-4 there, while on
    # the peaky logits of the same shape it loses more than that — the reason every regime is run
    _, p64, _, p32 = _case(regime='peaky').oracle()
    assert cc.K * v.e_ref < 1e-4 < cc.K * np.abs(p32 - p64).max()


def test_judge_notices_a_slab_shifted_by_a_frame_and_a_wrong_nll():
    for regime in cc.REGIMES:
        case = _case(regime=regime)
        n64, g64, _, _ = case.oracle()
        g = g64.copy()
        g[1, 1:] = g64[1, :-1]
        v = cc.judge(n64, g, case)
        assert not v.ok and 'gradient' in v.report and 'frame sums' not in v.report
        n = n64.copy()
        n[2] *= 1 + 4e-5
        v = cc.judge(n, g64, case)
        assert not v.ok and 'nll' in v.report and '[b 2]' in v.report and 'gradient' not in v.report
        g = g64.copy()
        g[0, 0, 0] = np.nan
        assert not cc.judge(n64, g, case).ok
    # grad_scale is divided out: the unscaled gradient of a scaled call is wrong
    case = _case(regime='random')
    n64, g64, _, _ = case.oracle()
    assert cc.judge(n64, g64 * 0.37, case, 0.37).ok and not cc.judge(n64, g64, case, 0.37).ok


def oracle_run(logits, logit_len, labels, label_len, scale, flaw=None):
    """CPU stand-in of ops.ctc_loss_grad for tests/ctc_kernel_check.exact_failures: float64 oracle, the kernel's
    clamping and its treatment of utterances without a valid alignment; `flaw` makes it wrong in one way"""
    B, T, C = logits.shape
    Lmax = labels.shape[1]
    nll = np.zeros(B, np.float32)
    dl = np.zeros((B, T, C), np.float32)
    status = 0
    oracle_run.calls += 1
    for b in range(B):
        Tb = min(max(int(logit_len[b]), 0), T)
        L = min(max(int(label_len[b]), 0), Lmax)
        if flaw == 'no clamp' and (logit_len[b] > T or label_len[b] < 0 or label_len[b] > Lmax):
            nll[b] = 1.0
            continue
        lab = labels[b:b + 1, :L]
        ok = Tb >= 1 and np.all((lab >= 0) & (lab < C - 1)) and L + int(np.sum(lab[0, 1:] == lab[0, :-1])) <= Tb
        if flaw == 'blank label accepted' and Tb >= 1 and np.any(lab == C - 1):
            nll[b], ok = 1.0, None
        if ok:
            n, g = O.ctc_loss(logits[b:b + 1].astype(np.float64), [Tb], lab, [L])
            nll[b], dl[b] = n[0], g[0] * scale
        elif ok is not None:
            nll[b] = np.inf
            status = status or b + 1
            if flaw == 'bad slab not cleared':
                dl[b, -1, -1] = 1e-3
            if flaw == 'wrong status':
                status = B + 1
    if flaw == 'timing':
        dl[0, 0, 0] = np.nextafter(dl[0, 0, 0], np.float32(9 if oracle_run.calls % 2 else -9))      # differs from call to call
    if flaw == 'neighbours' and B > 1:
        dl[1, 0, 0] += np.float32(1e-7) * np.float32(logits[0, 0, 0])
    if flaw == 'bad neighbour leaks' and status:
        dl[(status - 1 + 1) % B if B > 2 else 0, 0, 0] += np.float32(1e-3)
    if flaw == 'padding':
        dl[-1, T - 1, 0] = 1e-9
    if flaw == 'status':
        status = status or 1
    if flaw == 'nan':
        nll[0] = np.nan
    return nll, dl, status


oracle_run.calls = 0


def test_exact_checks_pass_on_the_reference_and_fail_on_every_flaw():
    import functools
    for shape, lattice in (((4, 40, 64, 10), 'loose'), ((3, 2, 3, 1), 'tight'), ((1, 1, 2, 0), 'loose'), ((2, 1, 2, 1), 'tight')):
        case = _case(shape, 'random', lattice)
        assert kc.exact_failures(case, 0.5, oracle_run(*case, 0.5), run=oracle_run) == []
    case = _case((4, 40, 64, 10), 'random', 'loose')     # last utterance shorter than T (checked below)
    assert case.logit_len[-1] < 40
    for flaw, word in (('timing', 'second call'), ('neighbours', 'reversing'), ('no clamp', 'clamped'),
                       ('blank label accepted', 'not +inf'), ('bad slab not cleared', 'not all zero'),
                       ('wrong status', 'names none'), ('bad neighbour leaks', 'valid utterance'),
                       ('padding', 'past its length'), ('status', 'on a valid batch'), ('nan', 'non-finite')):
        run = functools.partial(oracle_run, flaw=flaw)
        bad = kc.exact_failures(case, 1.0, run(*case, 1.0), run=run)
        assert any(word in b for b in bad), (flaw, bad)
    # a negative label_len on a batch of fewer than three utterances takes the branch of its own
    case = _case((2, 1, 2, 1), 'random', 'loose')
    run = functools.partial(oracle_run, flaw='no clamp')
    assert any('negative label_len' in b for b in kc.exact_failures(case, 1.0, run(*case, 1.0), run=run))
