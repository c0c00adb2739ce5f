"""nabu_pk_amax on both of its kernels: the routed library in this process, the atomic kernel for every shape
(NABU_PK_AMAX_ATOMIC=1, read once per process) in a child process.  Cases and what a source holds:
tests/pk_amax_routes_check.py.  Maxima are exact: everything is compared as integers, without a tolerance —
against NumPy, between the two routes, and the words around the destinations against their pattern.  The pair form
of the kernels is internal and is held to the same through the f16x3 BLSTM layer: outputs, dx and the four
gradients under the two routes, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pk_amax_routes_check as pc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def atomic(tmp_path_factory):
    """every case on the atomic kernel: one child process"""
    assert os.environ.get('NABU_PK_AMAX_ATOMIC', '0') in ('', '0'), 'NABU_PK_AMAX_ATOMIC is set: this process would not route'
    path = str(tmp_path_factory.mktemp('pk_amax') / 'atomic.npz')
    e = dict(os.environ)
    e['NABU_PK_AMAX_ATOMIC'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'pk_amax_routes_check.py'), path], env=e, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and 'PK AMAX CHILD OK' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return np.load(path)


def test_both_kernels_are_reached():
    """the routing rule, restated in pc.owned, sends a known part of the table to each kernel: a later change of the
    threshold may not quietly leave one of them without cases"""
    shapes = sorted(set(c[:2] + (c[3],) for c in pc.cases()))
    own = [c for c in shapes if pc.owned(*c)]
    assert len(shapes) == 5 * 7 * 3 and len(own) == 30, (len(shapes), own)
    for mode in pc.MODES:      # every mode on both kernels; the C = 262 tail on both; one block and several
        assert any(pc.owned(R, C, mode) for R, C, _ in shapes) and not all(pc.owned(R, C, mode) for R, C, _ in shapes)
        assert pc.owned(513, 262, mode) and not pc.owned(255, 262, 'cols') and pc.owned(513, 2048, mode)
    src = open(os.path.join(os.path.dirname(HERE), 'nabu_amd', 'csrc', 'gemm_pk.hip')).read()
    assert 'constexpr int PK_AMAX_PER_WORD = 2, PK_AMAX_MAX_COL = 8192, PK_AMAX_MIN_C = 256;' in src
    assert 'return atomics > PK_AMAX_PER_WORD * words;' in src


@pytest.mark.parametrize('R', pc.ROWS)
@pytest.mark.parametrize('C', pc.COLS)
def test_pk_amax_equals_numpy_on_both_routes(R, C, atomic):
    """all leading dimensions, modes and prefills of one shape"""
    todo = [c for c in pc.cases() if c[:2] == (R, C)]
    assert len(todo) == 2 * len(pc.MODES) * len(pc.PREFILLS)
    for c in todo:
        _, _, ld, mode, pre = c
        x = pc.source(R, C, ld)
        want = pc.expected(x, C, pc.prefill(R, pre), pc.prefill(C, pre))
        assert np.isnan(x[:, :C]).sum() == 1
        got = pc.run(c)
        for name, n, buf, w in zip(('rows', 'cols'), (R, C), got, want):
            if mode not in (name, 'both'):
                assert buf is None
                continue
            key = pc.case_id(c) + '/' + name
            np.testing.assert_array_equal(buf[pc.GUARD:pc.GUARD + n], w, err_msg=key)
            np.testing.assert_array_equal(buf[:pc.GUARD], pc.SENTINEL, err_msg=key + ': words in front')
            np.testing.assert_array_equal(buf[pc.GUARD + n:], pc.SENTINEL, err_msg=key + ': words behind')
            np.testing.assert_array_equal(atomic[key], buf, err_msg=key + ': the two routes differ')
            assert w.max() > 0x7F800000, 'the NaN did not reach the expected maxima'


@pytest.mark.parametrize('c', pc.layer_cases(), ids=[pc.layer_id(c) for c in pc.layer_cases()])
def test_blstm_layer_same_bits_under_both_routes(c, atomic):
    got = pc.run_layer(c)
    for k in pc.LAYER_KEYS:
        assert np.all(np.isfinite(got[k])), k
        np.testing.assert_array_equal(got[k].view(np.int32), atomic[pc.layer_id(c) + '/' + k].view(np.int32), err_msg=k)
