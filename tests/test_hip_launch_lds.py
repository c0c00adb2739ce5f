"""The launch helper's table of dynamic-LDS grants (csrc/common.hip: ensure_dynamic_lds) grows, is shared by all
threads and is kept per device: tests/launch_lds_check.py, run once as a child process so that the table starts empty.
A wrong table shows as an error return from a launch (more LDS than the function's attribute allows), not as a fault."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def child():
    r = subprocess.run([sys.executable, os.path.join(HERE, 'launch_lds_check.py')], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-4000:])
    return r


def steps(r, dev):
    return [ln for ln in r.stdout.splitlines() if ln.startswith('STEP %d ' % dev)]


def test_grant_grows_and_a_second_thread_does_not_lower_it(child):
    """64.4 KiB, 149.9 KiB, 64.4 KiB from a fresh thread, 149.9 KiB again: status 0 and judge() on every call"""
    assert child.returncode == 0 and 'LDS OK' in child.stdout, (child.stdout[-4000:], child.stderr[-2000:])
    lines = steps(child, 0)
    assert len(lines) == 4 and all(ln.endswith(' OK') for ln in lines), lines
    assert [ln.split()[-2] for ln in lines] == ['main', 'main', 'thread', 'main']
    assert [int(ln.split()[4]) > 64 * 1024 for ln in lines] == [True] * 4


def test_the_same_on_a_second_device_of_the_process(child):
    """the grants of device 0 say nothing about device 1: the same four steps there, in the same process"""
    skipped = [ln for ln in child.stdout.splitlines() if ln.startswith('DEVICE 1 SKIPPED')]
    if skipped:
        pytest.skip(skipped[0])
    assert child.returncode == 0 and 'LDS OK' in child.stdout, (child.stdout[-4000:], child.stderr[-2000:])
    lines = steps(child, 1)
    assert len(lines) == 4 and all(ln.endswith(' OK') for ln in lines), lines
