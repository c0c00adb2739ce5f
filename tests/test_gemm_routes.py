"""No device: the case table of tests/gemm_routes.py against its restatement of the product dispatcher, and the
restatement against the one thing the library tells about its split decision, nabu_gemm_ws_bytes."""
import numpy as np
import pytest

from tests import gemm_routes as G


def _lib():
    from nabu_amd import _hip
    return _hip.lib()           # loads without a device (tests/test_abi.py)


@pytest.mark.parametrize('case', G.CASES, ids=repr)
def test_every_case_reaches_the_route_it_claims(case):
    for beta in (0.0, 1.0, 2.0):
        assert G.case_route(case, beta) == case.claimed(beta), (case, beta)
    if case.route0 != case.route:
        assert case.route0 == 'narrow'


def test_every_route_is_reached(capsys):
    reached = {}
    for c in G.CASES:
        for beta in (0.0, 2.0):
            reached.setdefault(G.case_route(c, beta), []).append('%s(beta=%g)' % (c.name, beta))
    with capsys.disabled():
        print()
        for r in sorted(reached):
            print('route %-30s reached by %s' % (r, ', '.join(reached[r])))
    assert set(G.ROUTES) <= set(reached), sorted(set(G.ROUTES) - set(reached))
    assert set(reached) <= set(G.ROUTES), 'a route nobody listed: %s' % sorted(set(reached) - set(G.ROUTES))
    # every kernel of the family, each transpose of the two tile kernels, and the reduce behind each kind of head
    kinds = {(r, c.ta, c.tb) for c in G.CASES for r in (c.route, c.route0)}
    for kernel in ('fast32 x1', 'generic x1'):
        for ta in (False, True):
            for tb in (False, True):
                assert (kernel, ta, tb) in kinds, (kernel, ta, tb)


def test_windows_do_not_overlap_their_guards():
    """the layout itself: every index inside its buffer, GUARD whole rows before the first and after the last, no two
    elements at one place, and the alignment flags are those of the pointers"""
    for c in G.CASES:
        L = G.layout(c)
        ia, ib, ic = G.indices(c, L)
        for idx, size, ld in ((ia, L['a_size'], L['lda']), (ib, L['b_size'], L['ldb']), (ic, L['c_size'], L['ldc'])):
            if idx.size == 0:
                continue
            assert idx.min() >= G.GUARD * ld and idx.max() < size - G.GUARD * ld, c
            assert np.unique(idx).size == idx.size, c
        for flag, ld, off in zip(L['aligned'], (L['lda'], L['ldb'], L['ldc']), (c.a_off, c.b_off, 0)):
            if ld % 4 == 0:         # rows of whole 16-byte pieces: only the window's own offset can misalign it
                assert flag == (off % 4 == 0), c


@pytest.mark.parametrize('case', G.CASES, ids=repr)
def test_workspace_holds_the_restated_slices(case):
    """nabu_gemm_ws_bytes knows M, N and K only: it is the largest of the split the tile kernels take at K, at
    K - K % 16 (the K-tail composition) and of the skinny kernel's chunks, whether or not the call is one the skinny
    kernel takes (nothing transposed, A aligned).  So it holds the slices of every route; it equals 4 M N S where
    there is no K tail, unless the shape alone would be a skinny one with more chunks than the route has slices
    (the segmented-K cases here: 16 x 64, K = 1152 is 9 chunks of 128 for the skinny rule and 4 slices for the tile
    kernels) — there it equals 4 M N times that chunk count."""
    lib = _lib()
    M, N, K = case.M, case.N, case.K
    got = lib.nabu_gemm_ws_bytes(M, N, K)
    assert got == G.ws_bytes(M, N, K)
    for beta in (0.0, 2.0):
        r = G.case_route(case, beta)
        S = G.launch_slices(r)
        if S > 1:
            assert got >= 4 * M * N * S, (case, r)
        if not G.is_tail(r):
            kc = G.gemm_skinny_chunk(M, N, K)
            shape_only = K // kc if kc else 1
            S_ws = max(S, shape_only)
            assert got == (4 * M * N * S_ws if S_ws > 1 else 0), (case, r, got)
            if shape_only <= S:
                assert got == (4 * M * N * S if S > 1 else 0)


def test_reference_bound_holds_for_a_float32_evaluation():
    """the reference and its bound against NumPy's own float32 product on the host (whatever order its BLAS sums in),
    on the smaller fp32 cases: inside the bound, and not vacuously — the worst element uses a fair part of it"""
    worst = 0.0
    for c in G.CASES:
        if c.prec != 'f32' or c.M * c.N * c.K > 2 ** 21 or c.M * c.N == 0:
            continue
        a, b, c0, bias = G.operands(c)
        alpha, beta, _ = G.EPILOGUES[1]
        got = (np.float32(alpha) * (a @ b) + bias + np.float32(beta) * c0).astype(np.float64)
        ref, bound = G.reference(c, G.EPILOGUES[1])
        err = np.abs(got - ref)
        assert (err <= bound).all(), c
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert 0.01 < worst <= 1.0, worst
