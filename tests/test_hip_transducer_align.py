"""nabu_transducer_align (csrc/transducer_align.hip) against the restatement of tests/transducer_align_ref.py.

Cases and checks: tests/transducer_align_check.py.  On the exact grid every lb, ly and partial sum is exact in float32,
so state, frame, conf and score must equal the reference's element for element — that pins the tie rule and the
backtrace.  In this process the default dispatch runs (the wave route for U1 <= 64); ONE child process runs the
wave-eligible grid cases with NABU_TRANSDUCER_ALIGN_WORKGROUP=1 and the parent compares bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import transducer_align_check as ck
from tests import transducer_align_ref as ar
from tests import transducer_cases as tc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_default = {}          # shape -> the five outputs of the default dispatch (computed once, read by the forced check)


def _default_run(shape):
    if shape not in _default:
        _default[shape] = ck.run(*ck.grid_reference(shape).inputs)
    return _default[shape]


def _assert_equals_reference(out, ref, enc_len, label_len):
    state, frame, conf, score, status = out
    assert status == 0 == ref[4]
    assert state.dtype == np.int32 and frame.dtype == np.int32 and conf.dtype == np.float32 and score.dtype == np.float32
    assert np.array_equal(state, ref[0]), np.argwhere(state != ref[0])[:5]
    assert np.array_equal(frame, ref[1]), np.argwhere(frame != ref[1])[:5]
    for b in range(len(enc_len)):
        assert np.all(state[b, enc_len[b]:] == -1)
        assert np.all(frame[b, label_len[b]:] == -1) and np.all(conf[b, label_len[b]:] == 0)
    assert np.array_equal(conf.astype(np.float64), ref[2]), np.abs(conf - ref[2]).max()
    assert np.array_equal(score.astype(np.float64), ref[3]), (score, ref[3])


@pytest.mark.parametrize('shape', ck.GRID_SHAPES, ids=ck.shape_id)
def test_grid_paths_equal_the_reference_exactly(shape):
    """state and frame element for element, the tails -1 and 0, status 0, score and conf EQUAL to the restatement's (the
    grid is exact); frame is the first t with state[t] > i; two calls: same bits"""
    assert not ck.forced_workgroup(), 'NABU_TRANSDUCER_ALIGN_WORKGROUP is set: this test would not reach the wave route'
    case = ck.grid_reference(shape)
    f, g, enc_len, labels, label_len = case.inputs
    out = _default_run(shape)
    _assert_equals_reference(out, case.ref64, enc_len, label_len)
    for b in range(shape[0]):
        assert not ar.check_path(out[0][b], out[1][b], enc_len[b], label_len[b], shape[1], shape[3])
    again = ck.run(*case.inputs)
    assert again[4] == 0 and ck.same_bits(again[:4], out[:4]), 'second call differs from the first'


def test_workgroup_route_on_the_wave_routes_shapes(tmp_path):
    """the switch is read once per process: a fresh child runs the wave-eligible grid cases on the workgroup route;
    all five outputs must be the default dispatch's, bit for bit"""
    todo = [s for s in ck.GRID_SHAPES if ck.wave_eligible(s[3])]
    assert len(todo) >= 8
    path = str(tmp_path / 'forced.npz')
    e = dict(os.environ)
    e['NABU_TRANSDUCER_ALIGN_WORKGROUP'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'transducer_align_check.py'), path], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ALIGN DONE' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    with np.load(path) as forced:
        for shape in todo:
            key = ck.shape_id(shape)
            out = _default_run(shape)
            assert int(forced[key + '/status']) == out[4] == 0, key
            for name, a in zip(ck.NAMES[:4], out[:4]):
                assert ck.same_bits([a], [forced['%s/%s' % (key, name)]]), '%s: %s differs between the routes' % (key, name)


@pytest.mark.parametrize('Lmax', [5, 70])
def test_constant_lattice_puts_every_label_at_frame_zero(Lmax):
    """f = g = 0: every path ties bit for bit; the tie rule alone puts every label at frame 0 (both routes' shapes)"""
    case = ar.constant_case(3, 30, 6, Lmax)
    f, g, enc_len, labels, label_len = case
    state, frame, conf, score, status = ck.run(*case)
    assert status == 0
    for b in range(3):
        Tb, Ub = int(enc_len[b]), int(label_len[b])
        assert np.all(frame[b, :Ub] == 0) and np.all(frame[b, Ub:] == -1)
        assert np.all(state[b, :Tb] == Ub) and np.all(state[b, Tb:] == -1)
        assert np.all(conf[b, :Ub] == conf[0, 0]) and abs(float(conf[0, 0]) + np.log(6.0)) < 1e-6


@pytest.mark.parametrize('entry', ck.CONTINUOUS, ids=['%dx%dx%dx%d-%s' % (s + (r,)) for s, r in ck.CONTINUOUS])
def test_continuous_logits(entry):
    """transducer_cases.make_case logits.  The device's path is a valid path with T_b blanks and U_b labels that ends
    in the final blank; its float64 value is >= the float64 best minus K_NLL times what the float32 restatement loses
    on its own best path (largest over the utterances) — where that is exactly 0, the floor 4 U sum|terms| stands in
    its place; score and conf: ck.scalar_allowances, the same allowance; and score <= -nll + allowance, with nll from
    ops.transducer_loss_grad on the same operands.  That allowance is WIDER than the one that holds score, by a second
    term: nll is itself a float32 kernel's number, held to its float64 value by transducer_cases.judge within K_NLL
    times the float32 loss restatement's error + 4 U (relative), and the inequality is exact only between the two
    float64 values.  So allowance = score's + nll's; the score's alone is printed beside it."""
    import torch
    from nabu_amd import ops
    shape, regime = entry
    B, T, C, Lmax = shape
    c = tc.make_case(B, T, C, Lmax, regime, tc.seed_of(*shape))
    case = tuple(c)
    f, g, enc_len, labels, label_len = case
    out = ck.run(*case)
    state, frame, conf, score, status = out
    assert status == 0
    for b in range(B):
        assert not ar.check_path(state[b], frame[b], enc_len[b], label_len[b], T, Lmax), b
    val64, _, sabs = ar.path_values(f, g, enc_len, labels, label_len, frame)
    _, fr64, _, best64, _, _ = ar.align(*case, dtype=np.float64)
    with np.errstate(over='ignore', under='ignore'):
        _, fr32, _, v32, _, _ = ar.align(*case, dtype=np.float32)
    own64, _, _ = ar.path_values(f, g, enc_len, labels, label_len, fr32)
    e32 = np.abs(v32.astype(np.float64) - own64)
    tol = tc.K_NLL * e32.max() if e32.max() > 0 else 4 * tc.U * sabs.max()
    print(entry, 'value gap %.3e, allowance %.3e (restatement %.3e)' % ((best64 - val64).max(), tol, e32.max()))
    assert np.all(val64 >= best64 - tol), (best64 - val64, tol)
    bad, figures, tol_abs = ck.scalar_allowances(case, out)
    print(entry, figures)
    assert not bad, (bad, figures)

    def dev(a, dtype):
        return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()
    nll = ops.transducer_loss_grad(dev(f, torch.float32), dev(g, torch.float32), dev(enc_len, torch.int32),
                                   dev(labels, torch.int32), dev(label_len, torch.int32), 1.0)[0].cpu().numpy()
    n64, _, _, n32, _, _ = c.reference()
    n_ref = float(np.max(np.abs(n32 - n64) / np.abs(n64)))
    allowance = tol_abs + (tc.K_NLL * n_ref + 4 * tc.U) * np.abs(n64)
    print(entry, 'score + nll at most %.3e, allowance at least %.3e (the score\'s alone %.3e)'
          % ((score + nll).max(), allowance.min(), tol_abs.min()))
    assert np.all(score.astype(np.float64) <= -nll.astype(np.float64) + allowance), (score, nll, allowance)


def _switch_T(U1, workgroup_route):
    """the largest T whose back-pointers and path still fit the LDS, by the implementation's own size function"""
    from nabu_amd import _hip
    L = _hip.lib()
    lo, hi = 1, 1 << 16
    assert L.nabu_transducer_align_lds_bytes(lo, U1, workgroup_route) <= ck.LDS_MAX
    assert L.nabu_transducer_align_lds_bytes(hi, U1, workgroup_route) > ck.LDS_MAX
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if L.nabu_transducer_align_lds_bytes(mid, U1, workgroup_route) <= ck.LDS_MAX:
            lo = mid
        else:
            hi = mid
    return lo, L.nabu_transducer_align_lds_bytes(lo, U1, workgroup_route), L.nabu_transducer_align_lds_bytes(hi, U1, workgroup_route)


@pytest.mark.parametrize('Lmax,workgroup_route', [(1, 0), (64, 1)], ids=['wave', 'workgroup'])
def test_backpointers_in_lds_and_in_the_workspace(Lmax, workgroup_route):
    """B = 1, C = 3, one grid case on each side of the switch that nabu_transducer_align_lds_bytes names (150 KiB):
      wave route, U1 = 2:        T = 12798: 12 * 12800 = 153600 B, in LDS;  T = 12799: 153612 B, in the workspace
      workgroup route, U1 = 65:  T = 7588: 528 + 20 * 7653 = 153588 B, in LDS;  T = 7589: 153608 B, in the workspace
    both must equal the restatement element for element (the sums stay exact: under 2^14 terms)"""
    assert not ck.forced_workgroup()
    T, fits, over = _switch_T(Lmax + 1, workgroup_route)
    assert (T, fits, over) == ((12798, 153600, 153612) if not workgroup_route else (7588, 153588, 153608))
    for t in (T, T + 1):
        inputs, ref = ck.grid_draw((1, t, 3, Lmax))
        assert ref[5].sum() >= 1
        out = ck.run(*inputs)
        _assert_equals_reference(out, ref, inputs[2], inputs[4])


def test_no_labels_at_all():
    """U1 = 1 (what transducer_decoder aligns when it recognised nothing): labels, frame and conf are null pointers;
    every state is 0 and the score is the sum of the blanks' log-probabilities"""
    c = tc.make_case(3, 9, 5, 0, 'random', 17)
    f, g, enc_len, labels, label_len = c
    state, frame, conf, score, status = ck.run(f, g, enc_len, None, label_len)
    ref = ar.align(f, g, enc_len, None, label_len)
    assert status == 0 == ref[4] and frame.shape == (3, 0) and conf.shape == (3, 0)
    assert np.array_equal(state, ref[0]) and np.all(state[0] == 0)
    # at most 9 terms of like sign, each a float32 node expression (expf, logf and three additions: a few ulp), and as
    # many roundings in the sum: 64 U relative is some three times that
    assert np.allclose(score, ref[3], rtol=64 * tc.U, atol=0)


def test_invalid_rows_beside_valid_ones():
    """ordinary rejected input: a label = C-1 and an enc_len of 0 between two good rows"""
    f, g, enc_len, labels, label_len = (a.copy() for a in ar.grid_case((4, 20, 7, 5)))
    label_len[:] = [4, 3, 5, 2]
    enc_len[:] = [20, 17, 20, 12]
    good = [ck.run(f[b:b + 1], g[b:b + 1], enc_len[b:b + 1], labels[b:b + 1], label_len[b:b + 1]) for b in (0, 3)]
    labels[1, 1] = 7 - 1                                   # row 1: the blank as a label
    enc_len[2] = 0                                         # row 2: no frames
    state, frame, conf, score, status = ck.run(f, g, enc_len, labels, label_len)
    ref = ar.align(f, g, enc_len, labels, label_len)
    assert status == 2 == ref[4]                           # the first rejected row
    for b in (1, 2):
        assert np.isneginf(score[b]) and np.all(state[b] == -1) and np.all(frame[b] == -1) and np.all(conf[b] == 0)
    for b, alone in zip((0, 3), good):
        assert alone[4] == 0
        assert ck.same_bits([state[b], frame[b], conf[b], score[b:b + 1]], [alone[0][0], alone[1][0], alone[2][0], alone[3]])
        assert np.array_equal(state[b], ref[0][b]) and np.array_equal(frame[b], ref[1][b]) and score[b] == ref[3][b]
    enc_len[2], labels[1, 1] = 9, 0
    assert ck.run(f, g, enc_len, labels, label_len)[4] == 0


def test_argument_checks_arrive_before_any_launch():
    """NABU_EINVAL and NABU_EWS: the outputs are untouched"""
    import torch
    from nabu_amd import _hip
    L = _hip.lib()
    B, T, U1, C = 2, 5, 3, 4
    dev = 'cuda'
    f, g = torch.zeros((B, T, C), device=dev), torch.zeros((B, U1, C), device=dev)
    enc_len, label_len = torch.full((B,), T, dtype=torch.int32, device=dev), torch.full((B,), 2, dtype=torch.int32, device=dev)
    labels = torch.zeros((B, U1 - 1), dtype=torch.int32, device=dev)
    state = torch.full((B, T), 77, dtype=torch.int32, device=dev)
    frame = torch.full((B, U1 - 1), 77, dtype=torch.int32, device=dev)
    conf, score = torch.full((B, U1 - 1), 77.0, device=dev), torch.full((B,), 77.0, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    need = L.nabu_transducer_align_ws_bytes(B, T, U1)
    assert need > 0 and L.nabu_transducer_align_ws_bytes(0, T, U1) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    p = _hip.ptr

    def call(B_=B, f_=f, labels_=labels, ldl=U1 - 1, ws_bytes=need, C_=C):
        return L.nabu_transducer_align(B_, T, U1, C_, p(f_) if f_ is not None else None, p(g), p(enc_len),
                                       p(labels_) if labels_ is not None else None, ldl, p(label_len), p(state), p(frame),
                                       p(conf), p(score), p(status), p(ws), ws_bytes, _hip.stream())
    assert call(B_=0) == -1 and call(f_=None) == -1 and call(labels_=None) == -1 and call(ldl=1) == -1 and call(C_=1) == -1
    assert call(ws_bytes=need - 1) == -3 and b'workspace' in L.nabu_last_error()
    torch.cuda.synchronize()
    for a in (state, frame, conf, score, status):
        assert bool((a == 77).all().item())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and bool((frame == 0).all().item())
