"""ctc_wave_split_kernel (alpha and beta sweeps side by side, gradient over frames after one barrier) against the
float64 oracle and against ctc_wave_kernel, which a child process runs under NABU_CTC_WAVE_SERIAL=1.

Cases: tests/ctc_split_check.py (the table of tests/ctc_cases.py plus T / L / C edges, short inputs, infeasible
pairs and a mixed batch).  Bounds: judge() of tests/ctc_cases.py with its own K and K_NLL, exactly as
tests/test_hip_ctc.py holds ctc_wave_kernel to them; the difference between the two kernels may not exceed the old
kernel's own distance to float64 on the same case.  (The new kernel evaluates the old one's expressions in the old
order; each case prints whether the bits agree.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ctc_cases as cc
from tests import ctc_split_check as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def old(tmp_path_factory):
    """every case on ctc_wave_kernel: one child process (the switch is read once per process)"""
    assert os.environ.get('NABU_CTC_WAVE_SERIAL', '0') in ('', '0'), 'NABU_CTC_WAVE_SERIAL is set: this process would not run the new kernel'
    path = str(tmp_path_factory.mktemp('ctc_split') / 'old.npz')
    e = dict(os.environ)
    e['NABU_CTC_WAVE_SERIAL'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'ctc_split_check.py'), path], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and 'CTC SPLIT CHILD OK' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return np.load(path)


def _sub(case, keep):
    """the utterances `keep` of a case as a case of their own (for the oracle)"""
    return cc.Case(case.logits[keep], case.logit_len[keep], case.labels[keep], case.label_len[keep], case.need[keep], case.meta)


def test_most_cases_reach_the_split_kernel():
    """sc.split_eligible restates ctc_split_lds_bytes and the dispatch: 174 of the 194 cases run the new kernel in this
    process (the others — two lattices over 150 KiB — run ctc_wave_kernel on both sides), among them cfg2's full size,
    lane 63 (L = 63) and every T, L and C of the grid; a later change of the rule may not quietly empty the comparison"""
    src = open(os.path.join(os.path.dirname(HERE), 'nabu_amd', 'csrc', 'ctc.hip')).read()
    for text in ('constexpr int CTC_SPLIT_WAVES = %d;' % sc.SPLIT_WAVES,
                 '((size_t)T * C + 2 * (size_t)T * Smax + CTC_SPLIT_WAVES * (64 + (size_t)C) + 2) * sizeof(float) + 128 * sizeof(int)',
                 '!force_wg && !serial && Lmax <= 63 && sshm <= 150 * 1024'):
        assert text in src, text
    took = [c for c in sc.CASES if sc.split_eligible(*sc.build(c).shape[1:])]
    assert len(sc.CASES) == 194 and len(took) == 174
    ids = set(c['id'] for c in took)
    assert 'table-32x125x40x60-random-loose' in ids and 'mixed' in ids and 'mixed-infeasible' in ids
    grid = [c['grid'] for c in took if 'grid' in c]
    for k, want in enumerate(((1, 2, 3, 64, 65), (0, 1, 31, 32, 63), (2, 40, 64, 300))):
        assert sorted(set(g[k] for g in grid)) == list(want)
    assert sc.split_eligible(65, 64, 63) and not sc.split_eligible(65, 300, 63)


@pytest.mark.parametrize('c', sc.CASES, ids=[c['id'] for c in sc.CASES])
def test_split_kernel_against_oracle_and_serial_kernel(c, old):
    from tests import ctc_kernel_check as kc
    assert not kc.forced_workgroup(), 'NABU_CTC_WORKGROUP is set: this test would not reach the wave kernels'
    case, scale = sc.build(c), c['scale']
    nll, dl, status = kc.run(case.logits, case.logit_len, case.labels, case.label_len, scale)
    nll2, dl2, status2 = kc.run(case.logits, case.logit_len, case.labels, case.label_len, scale)
    assert status2 == status and kc.same_bits(nll2, nll) and kc.same_bits(dl2, dl), 'two runs of the new kernel differ'
    onll, odl, ostatus = old[c['id'] + '/nll'], old[c['id'] + '/dl'], int(old[c['id'] + '/status'])

    bad = sc.infeasible(case)
    good = np.setdiff1d(np.arange(len(case.logit_len)), bad)
    if len(bad):      # the status word and the zero gradient of skipped utterances, as before
        assert status - 1 in bad and ostatus - 1 in bad, (status, ostatus, bad)
        assert np.all(np.isposinf(nll[bad])) and np.all(dl[bad] == 0)
        assert np.all(np.isposinf(onll[bad])) and np.all(odl[bad] == 0)
    else:
        assert status == 0 and ostatus == 0
    for b in range(len(case.logit_len)):
        assert np.all(dl[b, case.logit_len[b]:] == 0), 'utterance %d: gradient past its length' % b
    if not len(good):
        return
    sub = _sub(case, good) if len(bad) else case
    v_new = cc.judge(nll[good], dl[good], sub, scale)
    v_old = cc.judge(onll[good], odl[good], sub, scale)
    n64 = sub.oracle()[0]
    d_g = float(np.abs(dl[good].astype(np.float64) - odl[good].astype(np.float64)).max()) / scale
    d_n = float((np.abs(nll[good].astype(np.float64) - onll[good].astype(np.float64)) / np.abs(n64)).max())
    print('CASE %s split %s | new e %.3e s %.3e n %.3e | old e %.3e s %.3e n %.3e | new - old: gradient %.3e nll %.3e %s' % (
        c['id'], sc.split_eligible(case.shape[1], case.shape[2], case.shape[3]), v_new.e_ker, v_new.s_ker, v_new.n_ker,
        v_old.e_ker, v_old.s_ker, v_old.n_ker, d_g, d_n,
        'same bits' if kc.same_bits(nll, onll) and kc.same_bits(dl, odl) else 'DIFFERENT bits'))
    assert v_new.ok, v_new.report
    assert d_g <= v_old.e_ker, 'gradients of the two kernels differ by %.3e, the old one is %.3e from float64' % (d_g, v_old.e_ker)
    assert d_n <= v_old.n_ker, 'nll of the two kernels differs by %.3e, the old one is %.3e from float64' % (d_n, v_old.n_ker)
