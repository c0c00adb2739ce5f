"""GPU test of the parameter-update kernels against bits recorded on the device (tests/golden/update_bits.npz, written by
tests/golden/make_update_bits.py, which says where the numbers come from): clip, accumulate, the Adam step through its
four entry points, with the NaN factor that skips it.  The float64 tests bound the error of these kernels; this one pins
which products the Adam update fuses, in the 16-byte body and in the tail, which no error bound can see."""
import os

import numpy as np
import pytest

from tests.golden import make_update_bits as U

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'update_bits.npz')


@pytest.fixture(scope='module')
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_inputs_are_the_recorded_ones_and_hold_every_class(recorded):
    for n in U.SIZES:
        x = U.inputs(n)
        assert all(a.dtype == np.uint32 and a.shape == (n,) for a in x.values())
        np.testing.assert_array_equal(U.digest(x[k] for k in sorted(x)), recorded['%d|inputs' % n], err_msg='n = %d' % n)
    x = U.inputs(U.FULL)
    f = {k: a.view(np.float32) for k, a in x.items()}
    with np.errstate(invalid='ignore'):
        for _, scale in U.GRAD_SCALES:
            a = np.abs(f['g'] * np.float32(scale))
            assert (a > 1).sum() > 50 and (a < 1).sum() > 50
    assert np.isnan(f['g']).any() and np.isposinf(f['g']).any() and (x['g'] == 0x80000000).any()
    assert (f['m'] > 0).sum() > 100 and (f['m'] < 0).sum() > 100
    v = f['v']
    assert (x['v'] == 0).sum() > 100                                                                  # exactly 0,
    for lo, hi in ((2.0 ** -149, 2.0 ** -126), (2.0 ** -126, 2.0 ** -96), (2.0 ** -20, 8.0)):         # denormal, tiny, ordinary
        assert ((v >= lo) & (v < hi)).sum() > 100, (lo, hi)
    assert U.SIXTH == float(np.float32(1 / 6)) and [c for _, c in U.CLIPS] == [1.0, float('inf')]


def differences(n, name, arrays, recorded):
    """one line per array of a call that is not the recorded one"""
    out = []
    for k, t in arrays.items():
        want, got = recorded['%d|%s|%s' % (n, name, k)], U.bits(t)
        if n > U.FULL:
            got = U.digest([got])
            if not np.array_equal(got, want):
                out.append('%s, n = %d, %s: SHA-256 %s, recorded %s' % (name, n, k, got.tobytes().hex(), want.tobytes().hex()))
        elif not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            out.append('%s, n = %d, %s[%d] (the first of %d): 0x%08x, recorded 0x%08x'
                       % (name, n, k, i, int((got != want).sum()), got[i], want[i]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n', U.SIZES)
def test_the_update_kernels_write_the_recorded_bits(n, recorded):
    failed, names = [], []
    for name, arrays in U.cases(n):
        names.append(name)
        failed += differences(n, name, arrays, recorded)
    made = {'%d|%s|%s' % (n, name, k) for name in names for k in ('p', 'm', 'v', 'g', 'out')}
    assert {k for k in recorded if k.startswith('%d|' % n) and not k.endswith('|inputs')} <= made      # every recorded call ran
    assert len(names) == 16 + 8 + 8
    assert not failed, '%d arrays differ from the recording:\n%s' % (len(failed), '\n'.join(failed))


def test_the_recorded_skipped_steps_left_the_state_alone(recorded):
    """what the recorded skipped steps must be, from the inputs alone: m and v untouched, the parameter untouched or = src"""
    n = U.FULL
    x = U.inputs(n)
    for tail in ('', '_acc', '_src', '_src_acc'):
        for k in ('p', 'm', 'v'):
            np.testing.assert_array_equal(recorded['%d|adam_scaled_step:factor_nan%s|%s' % (n, tail, k)], x[k])
