"""Device side of tests/test_hip_gemm_pk_routes.py: one call of nabu_gemm_pk per case of tests/gemm_pk_cases.py, and
the child-process body for the two switches that are read once per process.

run(case) packs the operands on the device, runs the product into destinations that lie inside larger buffers —
GUARD words in front, rows of ldc floats of which the columns past the destination's width are padding, GUARD words
behind, everything outside the destination holding SENTINEL — and returns the raw bits of everything: the packed
operands, the row maxima, the destination buffers.  Nothing is judged here.

As a program: python tests/gemm_pk_routes_check.py split|var OUT.npz — the cases marked for that switch, under the
environment the parent set (NABU_PK_SPLIT=3 resp. NABU_PK_VAR=0)."""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

from tests import gemm_pk_cases as P  # noqa: E402

GUARD = 32
SENTINEL = 0x5A5A5A5A


def c_buffer(c, width, c0):
    """uint32 host image of one destination: [GUARD | M rows of ldc | GUARD], the window holding c0's columns (NaN
    where beta == 0), SENTINEL elsewhere"""
    host = np.full(GUARD + c.M * c.ldc + GUARD, SENTINEL, np.uint32)
    win = host[GUARD:GUARD + c.M * c.ldc].reshape(c.M, c.ldc)
    win[:, :width] = (np.full((c.M, width), np.nan, np.float32) if c0 is None else np.ascontiguousarray(c0)).view(np.uint32)
    return host


def split_buffer(c, host, width):
    """(window [M, width] as uint32, everything else as a flat uint32 array)"""
    keep = np.ones(host.size, bool)
    idx = GUARD + np.arange(c.M)[:, None] * c.ldc + np.arange(width)[None, :]
    keep[idx.ravel()] = False
    return host[idx], host[keep]


def run(c, direct=None):
    """-> {key: array}: 'pa<i>' / 'pb<i>' packed operands (uint16), 'aa<i>' / 'ab<i>' row maxima (uint32, f16x3),
    'c<i>' / 'd<i>' the buffers of C / C2 (uint32) of batch entry i, 'ws_bytes' what nabu_gemm_pk_ws_bytes
    asked for"""
    import ctypes
    import torch
    from nabu_amd import _hip, ops
    o, _ = P.operands(c)
    alpha, beta, with_bias = c.epi
    w1, w2 = c.widths
    out, pa, pb, cb, db = {}, [], [], [], []
    for i in range(c.nbatch):
        a, b = ops.PackedOperand(c.M, c.K, c.planes, 'cuda'), ops.PackedOperand(c.N, c.K, c.planes, 'cuda')
        a.buf.fill_(0x5A)
        b.buf.fill_(0x5A)
        ops.pk_pack(a, torch.tensor(o.a[i], device='cuda'), bound=o.bound_a)
        ops.pk_pack(b, torch.tensor(o.b[i], device='cuda'))
        pa.append(a)
        pb.append(b)
        c0 = o.c0[i] if beta != 0 else None
        cb.append(torch.from_numpy(c_buffer(c, w1, None if c0 is None else c0[:, :w1]).view(np.int32)).cuda())
        if w2:
            db.append(torch.from_numpy(c_buffer(c, w2, None if c0 is None else c0[:, w1:]).view(np.int32)).cuda())

    def window(buf):
        return buf.data_ptr() + 4 * GUARD

    bias = torch.from_numpy(o.bias[:w1].copy()).cuda() if with_bias else None
    bias2 = torch.from_numpy(o.bias[w1:].copy()).cuda() if with_bias and w2 else None
    # nabu_gemm_pk itself: ops.gemm_pk takes whole contiguous tensors only, and the destinations here are windows
    L = _hip.lib()
    d = _hip.PkGemmDesc()
    d.size = ctypes.sizeof(_hip.PkGemmDesc)
    d.planes, d.M, d.N, d.nkb, d.nbatch = c.planes, c.M, c.N, pa[0].nkb, c.nbatch
    assert d.nkb == P.pk_kblocks(c.K, c.planes) and pa[0].rows_pad == P.pk_rows_pad(c.M)
    for i in range(c.nbatch):
        d.A[i], d.B[i], d.C[i] = pa[i].buf.data_ptr(), pb[i].buf.data_ptr(), window(cb[i])
        d.C2[i] = window(db[i]) if w2 else None
        if c.planes == 2:
            d.a_amax[i], d.b_amax[i] = pa[i].amax.data_ptr(), pb[i].amax.data_ptr()
    d.a_rows_pad, d.b_rows_pad, d.a_planes, d.b_planes = pa[0].rows_pad, pb[0].rows_pad, c.planes, c.planes
    d.ldc, d.n_split = c.ldc, c.n_split
    d.bias, d.bias2 = _hip.ptr(bias), _hip.ptr(bias2)
    d.alpha, d.beta = alpha, beta
    d.direct = c.direct if direct is None else direct
    nbytes = L.nabu_gemm_pk_ws_bytes(ctypes.byref(d))
    out['ws_bytes'] = np.array([nbytes], np.int64)
    ws = _hip.Workspace.get(nbytes, 'cuda', 'gemm') if nbytes else None
    _hip.check(L.nabu_gemm_pk(ctypes.byref(d), _hip.ptr(ws), nbytes, _hip.stream()), 'nabu_gemm_pk')
    torch.cuda.synchronize()
    for i in range(c.nbatch):
        out['pa%d' % i] = pa[i].buf.cpu().numpy().view(np.uint16)
        out['pb%d' % i] = pb[i].buf.cpu().numpy().view(np.uint16)
        if c.planes == 2:
            out['aa%d' % i] = pa[i].amax.cpu().numpy().view(np.uint32)
            out['ab%d' % i] = pb[i].amax.cpu().numpy().view(np.uint32)
        out['c%d' % i] = cb[i].cpu().numpy().view(np.uint32)
        if w2:
            out['d%d' % i] = db[i].cpu().numpy().view(np.uint32)
    return out


def main(argv):
    which, path = argv
    cases = {'split': P.split_cases, 'var': P.var_cases}[which]()
    out = {}
    for c in cases:
        for k, v in run(c).items():
            out[c.name + '/' + k] = v
    np.savez(path, **out)
    print('GEMM PK CHILD OK %s %d cases' % (which, len(cases)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
