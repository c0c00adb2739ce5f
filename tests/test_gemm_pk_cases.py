"""No device: tests/gemm_pk_cases.py held to its promises — the table reaches every instantiation, route class and
edge it claims, the restated routing agrees with nabu_gemm_pk_ws_bytes, every grid case is order-independent, the
yardstick rejects the errors a reworked tile loop would make and accepts a float32 evaluation, and the
representation contract of f16x3 is what the pack arithmetic says it is."""
import ctypes
import os

import numpy as np
import pytest

from tests import gemm_pk_cases as P

GRID = [c for c in P.CASES if c.kind == 'grid']
DENSE = [c for c in P.CASES if c.kind == 'dense']


# ------------------------------------------------------------------------------------------------------- the table
def _reach():
    """(kernel, route class) -> names, over the parent's runs and the two child processes"""
    out = {}
    for c in P.CASES:
        runs = [('', P.route(c))]
        if c.split:
            runs.append(('+split3', P.route(c, split_env=P.SPLIT_ENV)))
        if c.var:
            runs.append(('+var0', P.route(c, var_env=0)))
        for tag, r in runs:
            cls = 'one slice' if r.nsplit == 1 else ('two slices' if r.nsplit == 2 else '>= 3 slices')
            out.setdefault((r.kernel, cls), []).append(c.name + tag)
    return out


def test_every_instantiation_and_route_class_is_reached(capsys):
    reach = _reach()
    with capsys.disabled():
        print()
        for k in sorted(reach):
            print('gemm_pk_kernel<%d, %d> %-11s %2d: %s' % (k[0][0], k[0][1], k[1], len(reach[k]), ', '.join(reach[k])))
    plain = {(r.kernel, min(r.nsplit, 3)) for r in (P.route(c) for c in P.CASES)}
    # without an environment switch: all four reachable instantiations; one, two and >= 3 slices
    assert {k for k, _ in plain} == {(1, 0), (2, 0), (2, 1), (3, 1)}
    for kernel in ((1, 0), (2, 1), (3, 1)):
        assert (kernel, 1) in plain and (kernel, 2) in plain, kernel
    assert ((2, 1), 3) in plain
    # the children: the direct variant of bf16x6, the reduce pass behind every instantiation
    assert ((3, 0), 'one slice') in reach and ((3, 0), 'two slices') in reach
    for kernel in ((1, 0), (2, 0), (2, 1), (3, 1)):
        assert (kernel, '>= 3 slices') in reach, kernel


def test_slices_stages_and_the_direct_rule():
    routes = {c.name: P.route(c) for c in P.CASES}
    forced = {c.name: P.route(c, split_env=P.SPLIT_ENV) for c in P.split_cases()}
    # the ring's fill and drain: reductions of 1, 2, 3, 4, 5 and 7 stages in one slice (f16x3), 1 / 3 / 5 (one plane)
    for planes, want in ((2, {1, 2, 3, 4, 5, 7}), (3, {1, 2, 3, 7}), (1, {1, 3, 5})):
        got = {r.stages[0] for c, r in zip(P.CASES, routes.values()) if c.planes == planes and r.nsplit == 1}
        assert want <= got, (planes, got)
    # natural split-K: uneven last slices, >= 3 slices, a bf16x6 split, a one-plane split
    assert routes['g2-split2'].stages == [49, 48] and routes['g2-split3'].stages == [49, 49, 47]
    assert routes['g3-split2-sparse'].stages == [25, 24] and routes['g1-split2'].stages == [24, 24]
    assert routes['d3-k1000'].stages == [32, 31]
    # the child's NABU_PK_SPLIT=3: slices of one and of two stages, an uneven last slice, on edge tiles
    assert forced['g2-st3-129x68'].stages == [1, 1, 1] and forced['g2-st5-257x260'].stages == [2, 2, 1]
    assert forced['g1-st5'].stages == [2, 2, 1] and forced['g3-st7-sparse'].stages == [3, 3, 1]
    assert any(r.nsplit >= 3 and (c.M % 256 or c.N % 256) for c, r in ((P.BY_NAME[n], r) for n, r in forced.items()))
    # both outcomes of the direct = 2 rule, on the grid and on dense operands
    rule = {c.name: routes[c.name].direct for c in P.CASES if c.direct == 2}
    assert rule == {'g2-st2-31x60': True, 'g2-k4000': False, 'd2-rule-direct': True, 'd2-rule-promoted': False}
    assert {c.direct for c in P.CASES if c.planes == 2} == {0, 1, 2}


def test_edges_of_the_table():
    Ms, Ns = {c.M for c in P.CASES}, {c.N for c in P.CASES}
    assert {1, 31, 129, 256, 257, 300} <= Ms and {4, 60, 68, 256, 260, 516} <= Ns
    assert all(c.N % 4 == 0 for c in P.CASES)
    five = P.BY_NAME['g2-5x3-tiles']
    r = P.route(five)
    assert (r.tiles_m, r.tiles_n) == (5, 3) and r.tiles_m % P.PK_GM and (r.tiles_m * r.tiles_n) % 8
    assert {40, 1000} <= {c.K for c in P.CASES if c.K % 16}
    assert P.pk_kblocks(100, 1) == 9 and (100 + 15) // 16 == 7 and P.BY_NAME['g1-roundup'].K == 100
    assert any(c.nbatch == 2 and c.planes == p for c in P.CASES for p in (2,)) and any(c.nbatch == 2 and c.planes == 3 for c in P.CASES)
    two = [c for c in P.CASES if c.n_split]
    assert {c.planes for c in two} >= {2, 3} and all(c.ldc > max(c.widths) and c.epi[2] for c in two)
    assert any(c.n_split and c.nbatch == 2 for c in P.CASES)
    for planes in (1, 2, 3):          # alpha / beta / bias on and off; beta == 0 (a NaN-filled C) for every arithmetic
        epis = {c.epi for c in P.CASES if c.planes == planes}
        assert any(e[1] == 0 for e in epis) and any(e[1] != 0 and e[2] for e in epis)
    assert {P.E0, P.E1, P.E2, P.E3} <= {c.epi for c in P.CASES if c.planes == 2}
    assert all(c.M <= 1100 and c.N <= 516 and c.K <= 4000 for c in P.CASES)
    assert all(c.K <= 1024 for c in DENSE)
    assert all(c.K <= 48 or c.nnz for c in GRID if c.planes == 3)
    # the thresholds the table is designed against, as the source states them
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nabu_amd', 'csrc', 'gemm_pk.hip')).read()
    for text in ('constexpr int PK_T = 256;', 'constexpr int PK_GM = 4;', 'd->planes == 2 ? 48 : 24', 'eff -= 0.01 * (ns - 1);',
                 'direct = (long long)p.kb_per_split * 16 <= 2 * (K / (ns32 > 0 ? ns32 : 1));', '#define PK_RING2 3'):
        assert text in src, text


def _desc(c):
    from nabu_amd import _hip
    d = _hip.PkGemmDesc()
    d.size = ctypes.sizeof(_hip.PkGemmDesc)
    d.planes, d.M, d.N, d.nkb, d.nbatch = c.planes, c.M, c.N, P.pk_kblocks(c.K, c.planes), c.nbatch
    for i in range(c.nbatch):          # never dereferenced by nabu_gemm_pk_ws_bytes: any aligned non-null address
        d.A[i] = d.B[i] = d.C[i] = 0x1000
        d.C2[i] = 0x1000 if c.n_split else None
        if c.planes == 2:
            d.a_amax[i] = d.b_amax[i] = 0x1000
    d.a_rows_pad, d.b_rows_pad, d.a_planes, d.b_planes = P.pk_rows_pad(c.M), P.pk_rows_pad(c.N), c.planes, c.planes
    d.ldc, d.n_split, d.alpha, d.beta, d.direct = c.ldc, c.n_split, c.epi[0], c.epi[1], c.direct
    return d


@pytest.mark.parametrize('case', P.CASES, ids=repr)
def test_restated_split_is_the_librarys(case):
    """nabu_gemm_pk_ws_bytes is what the library tells about its split: 4 nsplit nbatch M N bytes, 0 for one slice.
    Without a device the library plans for 256 CUs (pk_cu_count), the count the table assumes."""
    from nabu_amd import _hip
    assert os.environ.get('NABU_PK_SPLIT', '') in ('', '-1', '0'), 'NABU_PK_SPLIT is set: the library would not route'
    got = _hip.lib().nabu_gemm_pk_ws_bytes(ctypes.byref(_desc(case)))
    assert got == P.ws_bytes(case), (case, got, P.route(case))


def test_restated_split_on_a_sweep_of_shapes():
    """the policy itself beyond the table: tile counts 1 .. 40, reductions up to 4096, every arithmetic"""
    from nabu_amd import _hip
    L = _hip.lib()
    n = 0
    for planes in (1, 2, 3):
        for M, N in ((256, 256), (257, 260), (300, 516), (1100, 516), (2048, 1280)):
            for K in (16, 700, 768, 784, 1152, 1536, 1552, 2304, 2320, 3000, 4096):
                for nbatch in (1, 2):
                    c = P.Case('sweep', 'dense', planes, M, N, K, P.E0, 'normal', nbatch=nbatch)
                    assert L.nabu_gemm_pk_ws_bytes(ctypes.byref(_desc(c))) == P.ws_bytes(c), (planes, M, N, K, nbatch)
                    n += P.route(c).nsplit > 1
    assert n > 40          # not vacuous: many of them split


# ------------------------------------------------------------------------------------------- grid cases: exactness
@pytest.mark.parametrize('case', GRID, ids=repr)
def test_grid_case_is_order_independent_and_exact(case):
    """operands() certifies the case (three float32 orders == float64, every plane non-zero, the epilogue exact); here
    also: the planes are those of the packed reference and y is a float32 number"""
    ops, pl = P.operands(case)
    for i in range(case.nbatch):
        y = P.value(case, i)
        assert P.exact_f32(y) and np.isfinite(y).all()
        (A, inv_a, packed, amax), _ = pl[0][i], pl[1][i]
        assert packed.shape == (P.pk_kblocks(case.K, case.planes), case.planes, P.pk_rows_pad(case.M), 16)
        if case.planes == 2:          # the scale element sets the row's scale: 2^14 scaled
            assert (np.abs(A[0]).max(axis=1) == 2.0 ** 14).all() and (case.M == 1 or len(set(inv_a)) > 1)
        if case.planes == 3:          # all 24 bits are held: the planes sum to the operand
            assert np.array_equal(sum(A)[:, :case.K], ops.a[i].astype(np.float64))
        if case.nnz:
            assert int((A[0] != 0).sum(axis=1).max()) <= 48          # terms per output


def test_subnormal_case_needs_the_subnormals():
    """flushing the l planes' fp16 subnormals to zero changes the bits of the result"""
    c = P.BY_NAME['g2-subnormal-l']
    y = P.value(c)
    flushed = P.value(c, drop=lambda A, B, pairs: A[1] @ B[0].T + A[0] @ B[1].T)
    assert (np.abs(P.operands(c)[1][0][0][0][1]).max() < 2.0 ** -14) and (y != flushed).mean() > 0.9


# ----------------------------------------------------------------------------------------- the yardstick has power
def _kslice(c, lo, hi):
    """drop: every kept plane product over k in [lo, hi)"""
    return lambda A, B, pairs: sum(A[x][:, lo:hi] @ B[y][:, lo:hi].T for x, y in pairs)


def mutations(c):
    """name -> float64 [M, N]: what a wrong kernel would hold for batch entry 0"""
    ops, pl = P.operands(c)
    A, B = pl[0][0][0], pl[1][0][0]
    y = P.value(c)
    M, N = y.shape
    m0, n0 = min(M - 1, 37), min(N - 1, 41)
    out = {}
    # one term: the one of median magnitude among the non-zero terms of (m0, n0)
    t = np.abs(sum(A)[m0] * sum(B)[n0])
    k0 = int(np.argsort(t)[(t == 0).sum() + (t != 0).sum() // 2])

    def one_term(A, B, pairs):
        d = np.zeros((M, N))
        d[m0, n0] = sum(A[x][m0, k0] * B[y][n0, k0] for x, y in pairs)
        return d
    out['one term dropped'] = P.value(c, drop=one_term)
    if c.planes > 1:
        # l.h (planes = 3: the lowest product, l.h) of one k-block in one 32 x 32 window
        kb = (P.pk_kblocks(c.K, c.planes) - 1) // 2
        r0, c0 = (m0 // 32) * 32, (n0 // 32) * 32

        def low_block(pair):
            def drop(A, B, pairs):
                d = np.zeros((M, N))
                x, yb = pair
                d[r0:r0 + 32, c0:c0 + 32] = (A[x][:, 16 * kb:16 * kb + 16] @ B[yb][:, 16 * kb:16 * kb + 16].T)[r0:r0 + 32, c0:c0 + 32]
                return d
            return drop
        out['l.h of one k-block dropped in one window'] = P.value(c, drop=low_block((c.planes - 1, 0)))
        if c.planes == 3:
            out['m.h of one k-block dropped in one window'] = P.value(c, drop=low_block((1, 0)))
    r = P.route(c, split_env=P.SPLIT_ENV if P.route(c).nsplit == 1 else -1)
    last = 16 * P.KBS[c.planes] * sum(r.stages[:-1])
    if r.nsplit > 1:
        out['last k-slice dropped'] = P.value(c, drop=_kslice(c, last, 16 * P.pk_kblocks(c.K, c.planes)))
    out['a row scale off by two'] = P.value(c, drop=lambda A, B, pairs: -np.where(np.arange(M)[:, None] == m0, P.plane_sum(A, B, pairs), 0.0))
    if M > 1:
        moved = y.copy()
        m1 = min(m0, M - 2)
        moved[m1 + 1] = y[m1]
        moved[m1] = ops.c0[0][m1] if c.epi[1] != 0 else np.nan          # what C held before the call
        out['a row written one row too far'] = moved
    return out


@pytest.mark.parametrize('case', DENSE, ids=repr)
def test_judge_accepts_float32_and_rejects_every_mutation(case):
    v = P.judge(case, P.value32(case))
    assert v.ok and v.ratio == pytest.approx(1.0)
    assert P.judge(case, P.value(case).astype(np.float32)).ok          # y rounded once
    if case.planes != 1:
        assert P.FLOOR < v.allowance < 64 * P.U, v          # the allowance is a few dozen u, not a norm-wise bar
    muts = mutations(case)
    want = {'one term dropped', 'a row scale off by two', 'a row written one row too far', 'last k-slice dropped'}
    assert want <= set(muts) and ((case.planes == 1) != ('l.h of one k-block dropped in one window' in muts))
    if case.planes == 3:
        # bf16x6's l.h is 2^-16 of a term: one k-block of it is below what float32 accumulation itself loses at any
        # reduction length, so no float32 yardstick sees it — the grid cases do (the test below); here the m.h product
        assert 'm.h of one k-block dropped in one window' in muts
        del muts['l.h of one k-block dropped in one window']
    for name, bad in muts.items():
        verdict = P.judge(case, bad.astype(np.float32))
        assert not verdict.ok, (case, name, verdict)


@pytest.mark.parametrize('case', GRID, ids=repr)
def test_every_mutation_changes_the_bits_of_a_grid_case(case):
    y = P.value(case).astype(np.float32)
    muts = mutations(case)
    assert len(muts) >= 3
    for name, bad in muts.items():
        assert not np.array_equal(y.view(np.uint32), bad.astype(np.float32).view(np.uint32)), (case, name)


# ------------------------------------------------------------------- the representation contract of f16x3, by itself
# x s = h + l with s = 2^(14 - floor(log2 ref)), ref = the row's largest magnitude or the a-priori bound:
#   h = rne16(x s): |x s - h| <= 2^-11 2^e for e = floor(log2 |x s|) >= -14 (11 significant bits), <= 2^-25 below (half
#       the spacing 2^-24 of fp16 subnormals);
#   l = rne16(x s - h): the residual is exact in float32; it is 2^(e-11) exactly (representable down to 2^-24) or has its
#       leading bit at 2^(e-12) or below, so |x s - h - l| <= 2^(e-23) <= 2^-23 |x s| — or 2^-25 where the residual is an
#       fp16 subnormal.  Hence  delta(x s) = |h + l - x s| <= max(2^-23 |x s|, 2^-25)   and   |l| <= 2^-11 |x s|
#       (rounding is monotone and 2^(e-11) is representable or l = 0).
# A kept term is (h_a + l_a)(h_b + l_b) - l_a l_b, so against the true scaled product
#   |term - x_a s_a x_b s_b| <= delta_a |x_b s_b| + delta_b |x_a s_a| + delta_a delta_b + 2^-22 |x_a s_a| |x_b s_b|,
# the last summand being the dropped l.l product.  In bits: an element keeps 23 bits (relative error 2^-23) while
# |x s| >= 2^-2, i.e. down to 2^-16 .. 2^-17 below ref's power of two, and one bit less per binade below that:
# 39 - d bits at 2^-d below, 15 at 2^-24, 7 at 2^-32, none from 2^-39 on.  (2^-25 / 2^-2 = 2^-23: where the absolute
# term takes over from the relative one.)
def delta(xs):
    return np.maximum(2.0 ** -23 * np.abs(xs), 2.0 ** -25)


def bits_kept(depth):
    """significant bits of an element 2^-depth below the power of two of its row's scale reference"""
    return int(min(23, 39 - depth))


def _rows_at_depth(depth, rng, rows=8, K=64, ref_exp=3):
    """rows whose useful elements lie in [2^-depth, 2^(1-depth)) of 2^ref_exp, with one outlier 2^ref_exp at k = 0"""
    x = rng.uniform(1.0, 2.0, (rows, K)) * rng.choice([-1.0, 1.0], (rows, K)) * 2.0 ** (ref_exp - depth)
    x[:, 0] = 2.0 ** ref_exp
    return x.astype(np.float32)


@pytest.mark.parametrize('how', ['measured', 'bound'])
@pytest.mark.parametrize('depth', [16, 24, 32])
def test_f16x3_representation_contract(depth, how):
    rng = np.random.default_rng(depth)
    K, rows = 64, 8
    a = _rows_at_depth(depth, rng, rows, K)
    b = _rows_at_depth(depth, rng, rows, K)
    b[:, 0], b[:, 1] = 0.0, 8.0          # the outlier of a row meets a zero of the other operand
    a[:, 1] = 0.0
    if how == 'bound':                   # one shared scale for all rows (x_bound): no outlier needed, same depth below it
        a[:, 0] = b[:, 1] = 0.0
        ref = np.full(rows, 8.0, np.float32)
    else:
        ref = np.abs(a).max(axis=1)
        assert (ref == 8.0).all() and (np.abs(b).max(axis=1) == 8.0).all()
    _, ha, la, sa = P.pack_ref_f16(a, ref, 256, 4)
    _, hb, lb, sb = P.pack_ref_f16(b, ref, 256, 4)
    f = lambda z: z[:rows].astype(np.float64)
    ha, la, hb, lb, sa, sb = f(ha), f(la), f(hb), f(lb), f(sa), f(sb)
    xa, xb = a.astype(np.float64) * sa[:, None], b.astype(np.float64) * sb[:, None]
    assert (sa == 2.0 ** 11).all()       # 8 -> 2^14
    for x, h, l in ((xa, ha, la), (xb, hb, lb)):
        assert (np.abs(h + l - x) <= delta(x)).all() and (np.abs(l) <= 2.0 ** -11 * np.abs(x)).all()
    # the product: y of the restatement against the true float64 product, componentwise
    y = (ha @ hb.T + ha @ lb.T + la @ hb.T) / (sa[:, None] * sb[None, :])
    true = a.astype(np.float64) @ b.astype(np.float64).T
    da, db = delta(xa), delta(xb)
    bound = (da @ np.abs(xb).T + np.abs(xa) @ db.T + da @ db.T + 2.0 ** -22 * (np.abs(xa) @ np.abs(xb).T)) / (sa[:, None] * sb[None, :])
    bound += (K + 2) * 2.0 ** -53 * (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T)      # float64's own
    assert (np.abs(y - true) <= bound).all()
    # bits: every useful element is within 2^-bits of itself, and some element really is as far as a quarter of that
    use = np.ones(K, bool)
    use[:2] = False
    rel = (np.abs(ha + la - xa) / np.maximum(np.abs(xa), 1e-300))[:, use]
    bits = bits_kept(depth)
    assert bits == {16: 23, 24: 15, 32: 7}[depth]
    assert rel.max() <= 2.0 ** -bits
    assert rel.max() > 2.0 ** -(bits + 2), (depth, rel.max())
    # and the product of two such rows keeps about as many: relative to sum |a_k| |b_k|
    mag = np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)).T
    # (two representation errors of 2^-bits and the dropped l.l product's 2^-22, the second-order term on top)
    assert (np.abs(y - true) <= 2.0 ** -(bits - 2) * (1 + 2.0 ** -20) * mag).all()
