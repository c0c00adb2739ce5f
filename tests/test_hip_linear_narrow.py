"""GPU: the narrow-output linear layer (nabu_amd/csrc/linear_narrow.hip) — the forward kernel that nabu_gemm_ex takes
for N <= 64 columns, and nabu_linear_bwd_f32 (dx, dW, db from one pass) — against NumPy in float64.

Shapes: M in {1, 31, 33, 257} (one row; a partial 16-row tile; one row past two tiles; several row blocks with a ragged
tail), K in {4, 36, 40, 1028} (below one k-chunk / k-slice, not a multiple of either, several chunks and slices with a
tail), N in {4, 40, 64}; every operand with a leading dimension larger than its row (B and dy rows off the 16-byte
phase in one of the two calls of each kind, so both staging paths run at every shape); with and without bias; the
backward call with and without dx.  Outputs are filled with NaN first and the padding columns must keep it.

Error bound: the classical componentwise one, which holds for ANY order of summation (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 3.1): |fl(sum of n products) - exact| <= gamma_n * sum |a_i| |b_i| with
gamma_n = n u / (1 - n u), u = 2^-24.  n = K for C = A·B; K + 1 and |bias| added to the sum where a bias is added (one
more rounding); N for dx; M for dW and db, whose reduction runs over the M rows.  Inputs are standard normal, seeded;
the float64 reference takes the float32 inputs exactly.

The reference and its bound were exercised without a device against torch's float32 matmul on the CPU (the same
shapes, the same inputs): worst |error| / bound over all cases 0.62 (C, at K = 4), 0.64 (dx, at N = 4), 0.99 (dW, at
M = 1, where the "sum" is one product and the bound one rounding), 0.04 (db): a float32 evaluation sits inside the
bound, closest where the reduction is shortest, as the theory says it must.  On an MI355X the kernels gave 0.62, 0.64,
0.99 and 0.04 as well (pytest -s prints them; LABNOTES.md section 29).

Also here: bitwise repeatability of both entry points; a row's logits and dx computed alone (M = 1) equal, bit for
bit, that row of the M = 257 call; shapes the narrow kernels do not take (N = 68, K = 6, a pointer 4 bytes off) are
NABU_EUNSUP for nabu_linear_bwd_f32 and still right through ops.gemm; dnn_decoder.linear forward + backward with the
switch NABU_LINEAR_NARROW on (this process) and off (a process of its own: the switch is read once) agree within the
sum of the two paths' bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import linear_narrow_layer as layer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')
MS, KS, NS = (1, 31, 33, 257), (4, 36, 40, 1028), (4, 40, 64)


def gamma(n):
    return n * U / (1 - n * U)


def ref_fwd(A, B, bias):
    """(C in float64, componentwise bound of a float32 evaluation in any order)"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    C, mag = A64 @ B64, np.abs(A64) @ np.abs(B64)
    if bias is None:
        return C, gamma(A.shape[1]) * mag
    return C + bias.astype(np.float64), gamma(A.shape[1] + 1) * (mag + np.abs(bias.astype(np.float64)))


def ref_bwd(x, dy, W):
    """{name: (float64 value, bound)} of dx = dy W^T, dW = x^T dy, db = colsum(dy)"""
    x64, d64, W64 = x.astype(np.float64), dy.astype(np.float64), W.astype(np.float64)
    M, N = dy.shape
    return {'dx': (d64 @ W64.T, gamma(N) * (np.abs(d64) @ np.abs(W64).T)),
            'dW': (x64.T @ d64, gamma(M) * (np.abs(x64).T @ np.abs(d64))),
            'db': (d64.sum(0), gamma(M) * np.abs(d64).sum(0))}


def operands(M, K, N):
    """seeded standard normal x / A [M,K], W / B [K,N], dy [M,N], bias [N] (one set per shape, shared by the tests)"""
    rng = np.random.default_rng(1000003 * M + 1009 * K + N)
    return (rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32),
            rng.standard_normal((M, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32))


def padded(a, ld, fill=0.0):
    """device [rows, cols] view with row stride ld of a buffer that holds `fill` elsewhere; (buffer, view)"""
    rows, cols = a.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float32, device='cuda')
    view = buf[:, :cols]
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 16 == 0
    return buf, view


def out_view(rows, cols, ld):
    buf = torch.full((rows, ld), NAN, dtype=torch.float32, device='cuda')
    return buf, buf[:, :cols]


def check(name, got, want, bound, worst):
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all(), name
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    worst[name] = max(worst.get(name, 0.0), ratio)
    print('%s: worst error / bound %.3f' % (name, ratio))
    assert (err <= bound).all(), '%s: error / bound up to %.3f' % (name, ratio)


def lin_bwd_raw(M, K, N, x, ldx, dy, ldy, W, ldw, dx, lddx, dW, db):
    """nabu_linear_bwd_f32 as it stands (return code, no exception)"""
    from nabu_amd import _hip
    L = _hip.lib()
    nbytes = L.nabu_linear_bwd_ws_bytes(M, K, N)
    ws = _hip.Workspace.get(nbytes, 'cuda', 'gemm')
    return L.nabu_linear_bwd_f32(M, K, N, x.data_ptr(), ldx, dy.data_ptr(), ldy, W.data_ptr(), ldw,
                                 dx.data_ptr() if dx is not None else None, lddx, dW.data_ptr(), db.data_ptr(),
                                 ws.data_ptr(), nbytes, _hip.stream())


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('M', MS)
def test_forward_against_float64(M, K, N):
    from nabu_amd import ops
    A, B, _, bias = operands(M, K, N)
    _, a = padded(A, K + 4)
    worst = {}
    for use_bias, ldb in ((True, N + 4), (False, N + 1)):       # 16-byte rows of B / rows off their phase
        _, b = padded(B, ldb)
        cbuf, c = out_view(M, N, N + 3)
        bv = torch.tensor(bias, device='cuda') if use_bias else None
        ops.gemm(a, b, c, bias=bv, precision='f32')
        want, bound = ref_fwd(A, B, bias if use_bias else None)
        check('C', c.cpu().numpy(), want, bound, worst)
        assert torch.isnan(cbuf[:, N:]).all(), 'a word outside C was written'
        cbuf2, c2 = out_view(M, N, N + 3)
        ops.gemm(a, b, c2, bias=bv, precision='f32')
        assert torch.equal(c, c2), 'two runs differ'
        if use_bias:                                            # the default arithmetic (fp32) takes the same kernel
            cbuf3, c3 = out_view(M, N, N + 3)
            ops.gemm(a, b, c3, bias=bv)
            if ops.get_gemm_precision() == 'f32':
                assert torch.equal(c, c3)


@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('M', MS)
def test_backward_against_float64(M, K, N):
    from nabu_amd import ops
    X, W, DY, _ = operands(M, K, N)
    ref = ref_bwd(X, DY, W)
    _, x = padded(X, K + 4)
    _, w = padded(W, N + 2)
    worst = {}
    for with_dx, ldy in ((True, N + 1), (False, N + 4)):
        _, dy = padded(DY, ldy)
        dxbuf, dx = out_view(M, K, K + 8)
        dW = torch.full((K, N), NAN, device='cuda')
        db = torch.full((N,), NAN, device='cuda')
        assert ops.linear_bwd(x, dy, w, dW, db, dx if with_dx else None)
        check('dW', dW.cpu().numpy(), *ref['dW'], worst)
        check('db', db.cpu().numpy(), *ref['db'], worst)
        if with_dx:
            check('dx', dx.cpu().numpy(), *ref['dx'], worst)
            assert torch.isnan(dxbuf[:, K:]).all(), 'a word outside dx was written'
        else:
            assert torch.isnan(dxbuf).all(), 'dx was written although it was not asked for'
        dxbuf2, dx2 = out_view(M, K, K + 8)
        dW2 = torch.full((K, N), NAN, device='cuda')
        db2 = torch.full((N,), NAN, device='cuda')
        assert ops.linear_bwd(x, dy, w, dW2, db2, dx2 if with_dx else None)
        assert torch.equal(dW, dW2) and torch.equal(db, db2), 'two runs differ'
        if with_dx:
            assert torch.equal(dx, dx2), 'two runs differ'


@pytest.mark.parametrize('K,N', [(1028, 40), (36, 64), (40, 4)])
def test_a_row_does_not_depend_on_its_batch(K, N):
    """logits and dx of row r alone (M = 1) equal row r of the M = 257 call, bit for bit"""
    from nabu_amd import ops
    M = 257
    A, B, DY, bias = operands(M, K, N)
    _, a = padded(A, K + 4)
    _, b = padded(B, N + 4)
    _, dy = padded(DY, N + 4)
    bv = torch.tensor(bias, device='cuda')
    c = torch.empty((M, N), device='cuda')
    ops.gemm(a, b, c, bias=bv, precision='f32')
    dx = torch.empty((M, K), device='cuda')
    dW, db = torch.empty((K, N), device='cuda'), torch.empty((N,), device='cuda')
    assert ops.linear_bwd(a, dy, b, dW, db, dx)
    for r in (0, 15, 16, 130, 256):
        c1 = torch.empty((1, N), device='cuda')
        ops.gemm(a[r:r + 1], b, c1, bias=bv, precision='f32')
        assert torch.equal(c1[0], c[r]), 'logits of row %d' % r
        dx1 = torch.empty((1, K), device='cuda')
        assert ops.linear_bwd(a[r:r + 1], dy[r:r + 1], b, torch.empty((K, N), device='cuda'),
                              torch.empty((N,), device='cuda'), dx1)
        assert torch.equal(dx1[0], dx[r]), 'dx of row %d' % r


@pytest.mark.parametrize('case', ['N=68', 'K=6', 'offset'])
def test_unsupported_shapes_take_the_general_path(case):
    """N > 64, K % 4 != 0 and a pointer 4 bytes off: NABU_EUNSUP from nabu_linear_bwd_f32, False from ops.linear_bwd with
    nothing written, and the three products through ops.gemm / ops.colsum within the same bounds"""
    from nabu_amd import ops
    M, K, N = 33, 36, 40
    if case == 'N=68':
        N = 68
    elif case == 'K=6':
        K = 6
    X, W, DY, bias = operands(M, K, N)
    off = 1 if case == 'offset' else 0          # floats: every operand 4 bytes off its 16-byte phase

    def put(a):
        rows, cols = a.shape
        ld = cols + 4
        buf = torch.zeros(rows * ld + 4, dtype=torch.float32, device='cuda')
        v = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
        v.copy_(torch.tensor(a))
        return v
    x, w, dy = put(X), put(W), put(DY)
    if off:
        assert x.data_ptr() % 16 == 4
    dW = torch.full((K, N), NAN, device='cuda')
    db = torch.full((N,), NAN, device='cuda')
    dx = put(np.full((M, K), np.nan, np.float32))
    rc = lin_bwd_raw(M, K, N, x, x.stride(0), dy, dy.stride(0), w, w.stride(0), dx, dx.stride(0), dW, db)
    assert rc == ops.NABU_EUNSUP
    assert ops.linear_bwd(x, dy, w, dW, db, dx) is False
    assert torch.isnan(dW).all() and torch.isnan(db).all() and torch.isnan(dx).all()
    worst = {}
    c = put(np.full((M, N), np.nan, np.float32))
    ops.gemm(x, w, c, bias=torch.tensor(bias, device='cuda'), precision='f32')
    check('C', c.cpu().numpy(), *ref_fwd(X, W, bias), worst)
    ref = ref_bwd(X, DY, W)
    ops.gemm(x, dy, dW, trans_a=True, precision='f32')
    ops.colsum(dy.contiguous(), db)
    ops.gemm(dy, w, dx, trans_b=True, precision='f32')
    check('dW', dW.cpu().numpy(), *ref['dW'], worst)
    check('db', db.cpu().numpy(), *ref['db'], worst)
    check('dx', dx.cpu().numpy(), *ref['dx'], worst)


def test_workspace_and_argument_errors():
    from nabu_amd import _hip, ops
    L = _hip.lib()
    assert L.nabu_linear_bwd_ws_bytes(4000, 1024, 40) == 32 * (1024 * 40 + 40) * 4      # 16 k-slices x 32 row blocks
    assert L.nabu_linear_bwd_ws_bytes(1, 4, 4) == (4 * 4 + 4) * 4
    assert L.nabu_linear_bwd_ws_bytes(0, 4, 4) == 0
    t = torch.zeros(64, device='cuda')
    p = t.data_ptr()
    assert L.nabu_linear_bwd_f32(4, 4, 4, p, 4, p, 4, p, 4, None, 0, p, p, p, 16, _hip.stream()) == -3     # workspace
    assert L.nabu_linear_bwd_f32(4, 4, 4, None, 4, p, 4, p, 4, None, 0, p, p, p, 256, _hip.stream()) == -1
    assert L.nabu_linear_bwd_f32(4, 4, 4, p, 3, p, 4, p, 4, None, 0, p, p, p, 256, _hip.stream()) == -1    # ldx < K


def test_layer_with_the_switch_on_and_off(tmp_path):
    """dnn_decoder.linear at B*T = 66, F = 40, C = 9: NABU_LINEAR_NARROW=0 (the general tiles, three backward calls, in a
    process of its own) against this process; both are within their bound of float64, so they differ by at most the
    sum of the two"""
    assert os.environ.get('NABU_LINEAR_NARROW', '1') != '0'
    on = layer.run()
    path = str(tmp_path / 'off.npz')
    env = dict(os.environ, NABU_LINEAR_NARROW='0')
    r = subprocess.run([sys.executable, os.path.abspath(layer.__file__), path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and 'LAYER OK' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    off = dict(np.load(path))
    X, DY, _ = layer.inputs()
    X, DY = X.reshape(-1, layer.F), DY.reshape(-1, layer.C)
    W, b = on['W'], on['b']
    assert np.array_equal(W, off['W']) and np.array_equal(b, off['b'])
    want, bound = ref_fwd(X, W, b)
    ref = ref_bwd(X, DY, W)
    worst = {}
    for run in (on, off):
        check('out', run['out'].reshape(-1, layer.C), want, bound, worst)
        for name in ('dx', 'dW', 'db'):
            check(name, run[name].reshape(ref[name][0].shape), *ref[name], worst)
    for name, bnd in (('out', bound), ('dx', ref['dx'][1]), ('dW', ref['dW'][1]), ('db', ref['db'][1])):
        diff = np.abs(on[name].astype(np.float64) - off[name].astype(np.float64)).reshape(bnd.shape)
        assert (diff <= 2 * bnd).all(), name
