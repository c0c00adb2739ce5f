"""GPU: every route of the row-major products (nabu_gemm_ex, nabu_gemm2_f32; gemm.hip, gemm_skinny.hip, gemm_bf16.hip,
the narrow forward kernel) element by element against float64, on windows.

The cases, the route each one reaches, the operands (rows and columns scaled over 70 binary orders of magnitude) and
the componentwise bound gamma(K + S + 3) (|alpha| |A| |B| + |beta| |C0| + |bias|) (+ the plane kernels' operand
rounding) are those of tests/gemm_routes.py; tests/test_gemm_routes.py checks that table without a device.

Every operand and the result are windows inside larger buffers: rows of width + pad floats, two guard rows before and
after.  What surrounds an operand window holds NaN, so a value read from outside it poisons the result; what
surrounds the window of C holds a fixed bit pattern that must be there, bit for bit, after the call.  Each case runs
with alpha = 1, beta = 0 on a window of C full of NaN (beta == 0 must not read C) and with alpha = -0.5, beta = 2 and
a bias; cases with more than one k-slice twice, and the bits must agree.

pytest -s prints the worst error / bound of every route (LABNOTES.md section 33)."""
import numpy as np
import pytest
import torch

from tests import gemm_routes as G

pytestmark = pytest.mark.gpu

NAN = float('nan')
PATTERN = 0x4b1d4b1d            # what surrounds the window of C: a finite float, about 1.03e7
WORST = {}                      # route -> worst error / bound so far (printed as it grows)


def poisoned(size, idx, values, fill=NAN):
    """device buffer of `size` floats holding `fill`, with values at the flat offsets idx"""
    host = np.full(size, fill, np.float32)
    host[idx.ravel()] = values.ravel()
    return torch.tensor(host, device='cuda')


def c_buffer(size, idx, values):
    """the buffer of C: PATTERN everywhere, the window holding `values` (an array, or NaN if None)"""
    host = np.full(size, PATTERN, np.int32).view(np.float32).copy()
    host[idx.ravel()] = NAN if values is None else values.ravel()
    return torch.tensor(host, device='cuda')


def surroundings_intact(buf, idx):
    host = buf.cpu().numpy().view(np.int32)
    keep = np.ones(host.size, bool)
    keep[idx.ravel()] = False
    return bool((host[keep] == PATTERN).all())


def check(route, what, got, want, bound):
    assert np.isfinite(got).all(), '%s [%s]: %d elements are not finite' % (what, route, (~np.isfinite(got)).sum())
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / np.maximum(bound, 1e-300)
    worst = float(ratio.max()) if err.size else 0.0
    if worst > WORST.get(route, -1.0):
        WORST[route] = worst
    print('%-30s %-34s worst error / bound %.3f (so far on this route %.3f)' % (route, what, worst, WORST[route]))
    if not (err <= bound).all():
        m, n = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError('%s [%s]: %d of %d elements outside the bound, worst at (%d, %d): got %r, float64 %r, '
                             'error / bound %.3g' % (what, route, (err > bound).sum(), err.size, m, n, got[m, n],
                                                     want[m, n], worst))


def run_case(c, epilogue, prec=None, dev=None):
    """one call of ops.gemm on fresh windows; (result window [M, N] on the host, were C's surroundings left alone)"""
    from nabu_amd import ops
    alpha, beta, with_bias = epilogue
    L = G.layout(c)
    ia, ib, ic = G.indices(c, L)
    a, b, c0, bias = G.operands(c)
    if dev is None:
        dev = {}
    if 'a' not in dev:
        dev['a'] = poisoned(L['a_size'], ia, a)
        dev['b'] = poisoned(L['b_size'], ib, b)
        dev['bias'] = torch.tensor(bias, device='cuda')
    cbuf = c_buffer(L['c_size'], ic, c0 if beta != 0 else None)
    av, bv, cv = dev['a'][L['a_start']:], dev['b'][L['b_start']:], cbuf[L['c_start']:]
    for v, flag in zip((av, bv, cv), L['aligned']):
        assert (v.data_ptr() % 16 == 0) == flag
    ops.gemm(av, bv, cv, c.ta, c.tb, alpha=alpha, beta=beta, bias=dev['bias'] if with_bias else None,
             M=c.M, N=c.N, K=c.K, lda=L['lda'], ldb=L['ldb'], ldc=L['ldc'], kseg=c.kseg, a_seg=L['a_seg'],
             b_seg=L['b_seg'], precision=prec or c.prec)
    torch.cuda.synchronize()
    host = cbuf.cpu().numpy()
    return host[ic.ravel()].reshape(c.M, c.N), surroundings_intact(cbuf, ic)


@pytest.mark.parametrize('case', G.CASES, ids=repr)
def test_route_elementwise_on_windows(case):
    c, dev = case, {}
    for epilogue in G.epilogues(c):
        alpha, beta, with_bias = epilogue
        route = G.case_route(c, beta)
        assert route == c.claimed(beta)
        what = '%s alpha=%g beta=%g%s' % (c.name, alpha, beta, ' bias' if with_bias else '')
        got, intact = run_case(c, epilogue, dev=dev)
        assert intact, '%s [%s]: a word outside the window of C was written' % (what, route)
        want, bound = G.reference(c, epilogue)
        check(route, what, got, want, bound)
        if c.K == 0 and beta == 0:                     # C = bias, or 0: exactly, and no NaN of the old C in it
            assert not got.any()
        if G.slices(route) > 1:
            again, intact = run_case(c, epilogue, dev=dev)
            assert intact and np.array_equal(got.view(np.int32), again.view(np.int32)), \
                '%s [%s]: two runs differ' % (what, route)


def test_k0_with_beta0_is_the_bias():
    c = G.BY_NAME['K0']
    got, intact = run_case(c, (1.0, 0.0, True))
    assert intact
    assert np.array_equal(got, np.broadcast_to(G.operands(c)[3], got.shape))


@pytest.mark.parametrize('name', ['bf16-K48', 'bf16-M130', 'bf16-A-off', 'bf16-skinny'])
def test_refused_shapes_are_exact_fp32_bit_for_bit(name):
    """include/nabu_hip.h: shapes the bf16 kernels do not take (K % 32, M % 4, unaligned operands) 'silently use the
    exact fp32 kernel — never a lower precision than asked', and skinny products are exact fp32 whatever the requested
    precision: the same call at 'bf16' and at 'f32' gives the same bits"""
    c = G.BY_NAME[name]
    assert c.prec == 'bf16' and not G.case_route(c, 2.0).startswith('bf16')
    for epilogue in G.EPILOGUES:
        dev = {}
        low, _ = run_case(c, epilogue, prec='bf16', dev=dev)
        exact, _ = run_case(c, epilogue, prec='f32', dev=dev)
        assert np.isfinite(low).all()
        assert np.array_equal(low.view(np.int32), exact.view(np.int32)), (name, epilogue)


def test_bf16_really_is_lower_precision_where_it_is_taken():
    """the positive control of the test above: at 132 x 68 x 64 the 'bf16' result differs from the 'f32' one by more than
    2^-12 |A| |B| somewhere (an operand rounded to 8 bits is off by up to 2^-9 of itself)"""
    c = G.BY_NAME['bf16-NN']
    assert G.case_route(c, 0.0) == 'bf16 x1'
    dev = {}
    low, _ = run_case(c, G.EPILOGUES[0], prec='bf16', dev=dev)
    exact, _ = run_case(c, G.EPILOGUES[0], prec='f32', dev=dev)
    a, b, _, _ = G.operands(c)
    mag = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))
    assert (np.abs(low.astype(np.float64) - exact) > 2.0 ** -12 * mag).any()


def window(a, pad=4, fill=NAN):
    """device view [rows, cols] with row stride cols + pad inside a buffer with two guard rows before and after, `fill`
    (a float, or PATTERN's bits if None) around it; (buffer, view)"""
    rows, cols = a.shape
    ld = cols + pad
    if fill is None:
        host = np.full((rows + 2 * G.GUARD, ld), PATTERN, np.int32).view(np.float32).copy()
    else:
        host = np.full((rows + 2 * G.GUARD, ld), fill, np.float32)
    host[G.GUARD:G.GUARD + rows, :cols] = a
    buf = torch.tensor(host, device='cuda')
    return buf, buf[G.GUARD:G.GUARD + rows, :cols]


def gemm2_raw(M, N, K1, K2, a, b, a2, b2, c, beta, bias):
    """nabu_gemm2_f32 itself on strided views (ops.gemm2 takes whole contiguous tensors only)"""
    from nabu_amd import _hip
    L = _hip.lib()
    nbytes = L.nabu_gemm2_ws_bytes(M, N, K1, K2)
    ws = _hip.Workspace.get(nbytes, 'cuda', 'gemm2')
    for v in (a, b, a2, b2, c):
        assert v is None or (v.stride(1) == 1 and v.data_ptr() % 16 == 0)
    _hip.check(L.nabu_gemm2_f32(M, N, K1, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), K2,
                                a2.data_ptr() if K2 else None, a2.stride(0) if K2 else 0,
                                b2.data_ptr() if K2 else None, b2.stride(0) if K2 else 0, beta, c.data_ptr(),
                                c.stride(0), bias.data_ptr(), ws.data_ptr(), nbytes, _hip.stream()), 'nabu_gemm2_f32')


@pytest.mark.parametrize('M,N,K1,K2', G.GEMM2_SHAPES)
def test_gemm2_on_windows(M, N, K1, K2):
    """nabu_gemm2_f32, [A | A2] . [B ; B2] + beta C + bias with the split-K sum inside the launch: windows on all five
    tensors, beta = 0 on a NaN C and beta = 2, three calls in a row on the same workspace with equal bits (the tickets
    of a call are handed back)"""
    S = (K1 + K2) // G.gemm2_chunk(K1, K2)
    route = 'gemm2 x%d' % S
    for beta in (0.0, 2.0):
        (a, b, c0, bias), want, bound = G.gemm2_reference(M, N, K1, K2, beta)
        _, av = window(a[:, :K1])
        _, bv = window(b[:K1])
        a2v = window(a[:, K1:])[1] if K2 else None
        b2v = window(b[K1:])[1] if K2 else None
        bd = torch.tensor(bias, device='cuda')
        outs = []
        for _ in range(3):
            cbuf, cv = window(c0 if beta != 0 else np.full((M, N), np.nan, np.float32), fill=None)
            gemm2_raw(M, N, K1, K2, av, bv, a2v, b2v, cv, beta, bd)
            torch.cuda.synchronize()
            host = cbuf.cpu().numpy()
            outs.append(host[G.GUARD:G.GUARD + M, :N].copy())
            host.view(np.int32)[G.GUARD:G.GUARD + M, :N] = PATTERN
            assert (host.view(np.int32) == PATTERN).all(), 'a word outside the window of C was written'
        check(route, '%dx%dx(%d+%d) beta=%g' % (M, N, K1, K2, beta), outs[0], want, bound)
        for o in outs[1:]:
            assert np.array_equal(outs[0].view(np.int32), o.view(np.int32)), 'two runs differ'
