"""GPU: nabu_gemm_pk element by element on every route (csrc/gemm_pk.hip: the tile kernel's five instantiations, the
split-K reduce pass, two destinations, two batch entries), on the cases of tests/gemm_pk_cases.py, which
tests/test_gemm_pk_cases.py checks without a device.

Every case first shows that the device pack equals the host planes (so a product failure is the product's), then
  grid cases   the bits of C and C2 equal the bits of the restatement's float64 value: no tolerance;
  dense cases  judge(): every 32 x 32 window within 4 x what a float32 evaluation of the restatement loses, + 2 u;
and in both the words in front of, between the rows of and behind the destinations keep their pattern.

NABU_PK_SPLIT and NABU_PK_VAR are read once per process: tests/gemm_pk_routes_check.py runs as a child, once with
NABU_PK_SPLIT=3 (slices of one and two stages, the reduce pass on edge tiles) and once with NABU_PK_VAR=0 (the direct
variant of bf16x6), and writes what it got; this process judges it.  pytest -s prints every dense ratio
(LABNOTES.md section 35)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gemm_pk_cases as P
from tests import gemm_pk_routes_check as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _child(tmp_path_factory, which, env):
    for k in ('NABU_PK_SPLIT', 'NABU_PK_VAR'):
        assert os.environ.get(k, '') in ('', '-1'), '%s is set: this process would not route' % k
    path = str(tmp_path_factory.mktemp('gemm_pk') / (which + '.npz'))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, 'gemm_pk_routes_check.py'), which, path], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'GEMM PK CHILD OK' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return np.load(path)


@pytest.fixture(scope='module')
def forced_split(tmp_path_factory):
    return _child(tmp_path_factory, 'split', {'NABU_PK_SPLIT': str(P.SPLIT_ENV)})


@pytest.fixture(scope='module')
def forced_direct(tmp_path_factory):
    return _child(tmp_path_factory, 'var', {'NABU_PK_VAR': '0'})


def result(c, out, i):
    """(result [M, N] as uint32: the windows of C and C2 side by side, everything around them as one flat array)"""
    w1, w2 = c.widths
    win, rest = R.split_buffer(c, out['c%d' % i], w1)
    if w2:
        win2, rest2 = R.split_buffer(c, out['d%d' % i], w2)
        win, rest = np.concatenate([win, win2], axis=1), np.concatenate([rest, rest2])
    return np.ascontiguousarray(win), rest


def check(c, out, route, what):
    """one run of a case, from this process or a child's file, against the host"""
    ops, pl = P.operands(c)
    assert int(out['ws_bytes'][0]) == (4 * route.nsplit * c.nbatch * c.M * c.N if route.nsplit > 1 else 0), \
        '%s: the library split differently from the restatement (%s)' % (what, route,)
    for i in range(c.nbatch):
        for key, side in (('pa', pl[0][i]), ('pb', pl[1][i])):
            _, _, packed, amax = side
            np.testing.assert_array_equal(out['%s%d' % (key, i)].reshape(packed.shape), packed,
                                          err_msg='%s: the device pack of %s differs from the host planes' % (what, key))
            if amax is not None:
                np.testing.assert_array_equal(out['a%s%d' % (key[1], i)][:amax.size], amax.view(np.uint32), err_msg=what + ': row maxima')
        got, rest = result(c, out, i)
        np.testing.assert_array_equal(rest, R.SENTINEL, err_msg='%s: a word outside the destination was written' % what)
        if c.kind == 'grid':
            want = P.value(c, i).astype(np.float32)
            np.testing.assert_array_equal(got, want.view(np.uint32), err_msg='%s [%s]: not the exact value' % (what, route,))
        else:
            v = P.judge(c, got.view(np.float32), i)
            print('%-18s %-12s <%d,%d> x%d  worst window %6.2f u, float32 yardstick %5.2f u: ratio %.3f of %g'
                  % (c.name, what.split(' ', 1)[-1], route.kernel[0], route.kernel[1], route.nsplit, v.worst / P.U, v.yard / P.U,
                     v.ratio, P.YARD))
            assert v.ok, '%s [%s]: %s' % (what, route, v)


def test_the_device_has_the_compute_units_the_table_assumes():
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == P.NCU


@pytest.mark.parametrize('case', P.CASES, ids=repr)
def test_case_on_its_route(case):
    check(case, R.run(case), P.route(case), case.name + ' routed')


@pytest.mark.parametrize('case', [c for c in P.CASES if c.direct == 2], ids=repr)
def test_direct_rule_takes_the_restated_side(case):
    """direct = 2 gives the bits of the side the restated rule names; on dense operands the other side's bits differ
    (on the grid all three agree: every order is exact)"""
    want = P.route(case).direct
    auto, promoted, direct = (result(case, R.run(case, direct=m), 0)[0] for m in (2, 0, 1))
    assert np.array_equal(auto, direct if want else promoted)
    assert np.array_equal(promoted, direct) == (case.kind == 'grid')


@pytest.mark.parametrize('case', P.split_cases(), ids=repr)
def test_case_under_forced_split(case, forced_split):
    out = {k.split('/', 1)[1]: forced_split[k] for k in forced_split.files if k.startswith(case.name + '/')}
    check(case, out, P.route(case, split_env=P.SPLIT_ENV), case.name + ' NABU_PK_SPLIT=%d' % P.SPLIT_ENV)


@pytest.mark.parametrize('case', P.var_cases(), ids=repr)
def test_case_on_the_direct_variants(case, forced_direct):
    out = {k.split('/', 1)[1]: forced_direct[k] for k in forced_direct.files if k.startswith(case.name + '/')}
    route = P.route(case, var_env=0)
    assert route.kernel == (case.planes, 0)
    check(case, out, route, case.name + ' NABU_PK_VAR=0')
