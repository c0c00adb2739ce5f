"""Both CTC kernels of csrc/ctc.hip at their limits against the float64 oracle.

Cases, yardstick and the reasons for every shape: tests/ctc_cases.py; what is checked on a case:
tests/ctc_kernel_check.py.  In this process the default dispatch runs (ctc_wave_kernel wherever the shape allows it,
ctc_kernel for Lmax > 63 or more than 150 KiB of LDS); a child process per group of cases runs the same shapes with
NABU_CTC_WORKGROUP=1, i.e. on ctc_kernel.

The only tolerance is judge()'s: the error of the float32 oracle on the same case times K = 4 for gradients and frame
sums, times K_NLL = 16 for the nll (one number per utterance: tests/ctc_cases.py says why), plus a floor of a few
float32 roundings.  Measured on an MI355X (table: LABNOTES.md, "CTC kernels against the float32 oracle")."""
import os
import subprocess
import sys

import pytest

from tests import ctc_cases as cc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('entry', cc.CASES, ids=[e['id'] for e in cc.CASES])
def test_ctc_default_dispatch(entry):
    """every case of the table on the kernel the library chooses: the exact properties and judge().
    Worst measured error as a multiple of the float32 oracle's, ctc_wave_kernel (92 cases): gradient 3.77, frame sums
    4.00 (both at (2, 1, 2, 1), where the floor decides; 3.01 is the largest allowance any case needs), nll 6.89
    (needs 2.08).  ctc_kernel on the 26 cases only it can take: 2.33, 2.34, 3.89."""
    from tests import ctc_kernel_check as kc
    assert not kc.forced_workgroup(), 'NABU_CTC_WORKGROUP is set: this test would not reach the wave kernel'
    line, bad = kc.check_case(entry)
    print(line)
    assert not bad, (line, bad)


@pytest.mark.parametrize('group', cc.GROUPS)
def test_ctc_workgroup_kernel_on_the_wave_kernels_shapes(group):
    """the shapes ctc_wave_kernel takes, on ctc_kernel (NABU_CTC_WORKGROUP=1 is read once per process: a child
    process per group, one at a time, never restarted).
    Worst measured error as a multiple of the float32 oracle's, ctc_kernel over these 92 cases: gradient 3.77, frame
    sums 4.00 ((2, 1, 2, 1): the floor decides; largest allowance needed 3.22), nll 7.48 (needs 4.46)."""
    e = dict(os.environ)
    e['NABU_CTC_WORKGROUP'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'ctc_kernel_check.py'), group, '--forced'], env=e,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and 'CTC OK' in r.stdout, (group, r.stdout[-6000:], r.stderr[-2000:])
