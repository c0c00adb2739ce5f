"""The row-major products (nabu_gemm_ex / nabu_gemm_f32 / nabu_gemm2_f32): a restatement of the dispatcher's rules, a
table of cases that reaches every kernel and every composition of kernels behind the one entry point, and a float64
reference with a componentwise error bound.  Host code only: tests/test_gemm_routes.py checks the table against the
restatement and the restatement against nabu_gemm_ws_bytes without a device, tests/test_hip_gemm_routes.py runs the
cases on one.

route(...) restates nabu_amd/csrc/gemm.hip (nabu_gemm_ex, gemm_run and their predicates) and gemm_skinny_chunk of
gemm_skinny.hip; every helper below names the function it restates.  A route is written the way the dispatcher
composes it: 'fast32 x4' = gemm_f32_fast_kernel on 4 k-slices followed by gemm_splitk_reduce_kernel, 'generic x1',
'skinny x3', 'bf16x6 x8', 'smallk', 'narrow', 'tail[fast32 x4 + generic x1]' = the K-tail composition (the first call on
K - K % 16, the second one adds the rest with beta = 1), 'none' = M == 0 or N == 0 (nothing is launched).

Operands: seeded standard normal, row i of op(A) scaled by 2^((7 i) % 41 - 20), column j of op(B), of the bias and of
C0 by 2^((5 j) % 31 - 15): the elements of one result span 70 binary orders of magnitude, so an error metric relative
to the largest element would not see most rows and columns; the componentwise bound sees each element.

Bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1, as ref_fwd of
tests/test_hip_linear_narrow.py): a float32 evaluation of alpha * sum_k a_k b_k + beta * c0 + bias in ANY order, in
which no term passes through more than n roundings, is within gamma(n) * (|alpha| sum |a_k| |b_k| + |beta| |c0| +
|bias|) of the exact value, gamma(n) = n u / (1 - n u), u = 2^-24.  n = K + S + 3: at most K additions in a k-slice
(the products themselves are exact inside a fused multiply-add), S additions of slices (for a K-tail composition S
counts the slices of both calls; the second call's alpha * acc + 1 * C costs the first call's terms two more roundings
and K % 16 + its slice count >= 2), and three for alpha, the bias and beta * C.  The skinny kernels sum four
wave-partials of KC / 4 terms each before the slices: KC / 4 + 3 <= KC.  The plane kernels add what rounding the
operands to 1, 2 or 3 bf16 pieces costs (include/nabu_hip.h), relative to |alpha| sum |a_k| |b_k|: PLANE_TERM."""
import collections
import zlib

import numpy as np

U = 2.0 ** -24
BM = BN = 128          # gemm_args.h
FKT = 16               # gemm.hip: k-tile of gemm_f32_fast_kernel
FBK = 32               # gemm_args.h: k-tile of the bf16 kernels and the granule of a k-slice
SMALLK_MAX = 96        # gemm.hip
LN_MAXN = 64           # linear_narrow.hip

# precision -> relative error of a product of two operands rounded to that many bf16 pieces
PLANE_TERM = {'f32': 0.0,
              'bf16': 2.0 ** -8 + 2.0 ** -17,     # two operands at 2^-9 each
              'bf16x3': 2.0 ** -15,               # the header's "~2^-16", doubled
              'bf16x6': 2.0 ** -24}               # the dropped m.l, l.m and l.l products are below 2^-25


def gamma(n):
    return n * U / (1 - n * U)


# ---------------------------------------------------------------------------------------------- the dispatcher's rules
def choose_split(M, N, K):
    """gemm.hip choose_split: (number of k-slices, k-range of a slice)"""
    tiles = ((M + BM - 1) // BM) * ((N + BN - 1) // BN)
    ns = 1
    if tiles < 768 and K >= 1024:
        ns = (768 + tiles - 1) // tiles
        ns = max(1, min(ns, K // (512 if K >= 4096 else 256)))
    ks = (K + ns - 1) // ns
    ks = (ks + FBK - 1) // FBK * FBK
    return (K + ks - 1) // ks, ks


def gemm_skinny_chunk(M, N, K):
    """gemm_skinny.hip gemm_skinny_chunk: the largest of 256 / 128 / 64 that divides K, 0 = not a skinny shape"""
    if M > 64 or N % 32 != 0 or K < 64:
        return 0
    for kc in (256, 128, 64):
        if K % kc == 0:
            return kc
    return 0


def smallk_ok(ta, tb, M, N, K, lda, ldb, ldc, kseg, al_a, al_b, al_c):
    """gemm.hip smallk_ok (the bias is a tensor of its own in every case here: aligned)"""
    return (not ta and not tb and kseg == 0 and 8 <= K <= SMALLK_MAX and K % 4 == 0 and M >= 2048 and N >= 4 and
            N % 4 == 0 and al_a and lda % 4 == 0 and al_b and ldb % 4 == 0 and al_c and ldc % 4 == 0)


def fast_f32_ok(ta, tb, M, N, K, lda, ldb, a_seg, b_seg, al_a, al_b):
    """gemm.hip fast_f32_ok"""
    return (K > 0 and K % FKT == 0 and al_a and lda % 4 == 0 and a_seg % 4 == 0 and al_b and ldb % 4 == 0 and
            b_seg % 4 == 0 and (not ta or M % 4 == 0) and (tb or N % 4 == 0))


def bf16_fast(M, N, K, lda, ldb, a_seg, b_seg, al_a, al_b):
    """gemm.hip gemm_run: `fast` (with a.vecA and a.vecB written out)"""
    vec_a = al_a and lda % 4 == 0 and a_seg % 4 == 0
    vec_b = al_b and ldb % 4 == 0 and b_seg % 4 == 0
    return M % 4 == 0 and N % 4 == 0 and K > 0 and K % FBK == 0 and vec_a and vec_b


def narrow_ok(M, N, K, lda, al_a, al_b, al_c):
    """linear_narrow.hip linear_narrow_fwd_ok (with the switch NABU_LINEAR_NARROW at its default)"""
    return M > 0 and 0 < N <= LN_MAXN and K > 0 and K % 4 == 0 and lda % 4 == 0 and al_a and al_b and al_c


def _run(precision, ta, tb, M, N, K, lda, ldb, ldc, kseg, a_seg, b_seg, al):
    """gemm.hip gemm_run: the kernel of one call and its number of k-slices"""
    al_a, al_b, al_c = al
    ns = choose_split(M, N, K)[0] if K > 0 else 1
    kc = gemm_skinny_chunk(M, N, K) if (not ta and not tb and kseg == 0 and al_a and lda % 4 == 0) else 0
    if kc:
        ns = K // kc
    if (precision == 'f32' or K % FBK != 0) and smallk_ok(ta, tb, M, N, K, lda, ldb, ldc, kseg, al_a, al_b, al_c):
        return 'smallk'
    if kc:
        return 'skinny x%d' % ns
    if precision != 'f32' and bf16_fast(M, N, K, lda, ldb, a_seg, b_seg, al_a, al_b):
        return '%s x%d' % (precision, ns)
    if fast_f32_ok(ta, tb, M, N, K, lda, ldb, a_seg, b_seg, al_a, al_b):
        return 'fast32 x%d' % ns
    return 'generic x%d' % ns


def route(precision, ta, tb, M, N, K, lda, ldb, ldc, beta, kseg=0, a_seg=0, b_seg=0, aligned=True):
    """gemm.hip nabu_gemm_ex.  precision: 'f32' | 'bf16' | 'bf16x3' | 'bf16x6' | 'f16x3' (resolved: not 'default');
    aligned: True, or three flags (A, B, C) — is the base pointer 16-byte aligned"""
    al = (True, True, True) if aligned is True else tuple(bool(x) for x in aligned)
    if precision == 'f16x3':                  # packed operands only: row-major operands take bf16x6
        precision = 'bf16x6'
    assert precision in PLANE_TERM, precision
    assert kseg == 0 or (ta and not tb and K % kseg == 0)
    if M == 0 or N == 0:
        return 'none'
    if precision == 'f32' and not ta and not tb and beta == 0 and kseg == 0 and narrow_ok(M, N, K, lda, *al):
        return 'narrow'
    Kt = K % FKT
    Km = K - Kt
    if (precision == 'f32' and Kt != 0 and Km >= 4 * FKT and not (M <= 64 and not ta and not tb) and
            (kseg == 0 or Km // kseg == (K - 1) // kseg) and
            fast_f32_ok(ta, tb, M, N, Km, lda, ldb, a_seg, b_seg, al[0], al[1])):
        # (the second call's operands start Km reduction indices in: a multiple of 16 bytes under fast_f32_ok)
        return 'tail[%s + %s]' % (_run(precision, ta, tb, M, N, Km, lda, ldb, ldc, kseg, a_seg, b_seg, al),
                                  _run(precision, ta, tb, M, N, Kt, lda, ldb, ldc, 0, 0, 0, al))
    return _run(precision, ta, tb, M, N, K, lda, ldb, ldc, kseg, a_seg, b_seg, al)


def _slice_counts(r):
    parts = r[5:-1].split(' + ') if r.startswith('tail[') else [r]
    return [int(p.split(' x')[1]) if ' x' in p else (0 if p == 'none' else 1) for p in parts]


def slices(r):
    """S of the bound: the k-slices of a route, those of both calls of a K-tail composition together"""
    return sum(_slice_counts(r))


def launch_slices(r):
    """the largest number of k-slices of ONE call of a route: what the workspace must hold"""
    return max(_slice_counts(r))


def is_tail(r):
    return r.startswith('tail[')


def ws_bytes(M, N, K):
    """gemm.hip nabu_gemm_ws_bytes: an upper bound that knows the shape only (no transposes, no alignment)"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    ns = choose_split(M, N, K)[0]
    if K % FKT and K > FKT:
        ns = max(ns, choose_split(M, N, K - K % FKT)[0])
    kc = gemm_skinny_chunk(M, N, K)
    if kc:
        ns = max(ns, K // kc)
    return 4 * ns * M * N if ns > 1 else 0


# ------------------------------------------------------------------------------------------------------------ the cases
class Case(object):
    """One product.  route: what the call reaches with beta != 0; route0: with beta == 0 (the narrow kernel takes fp32
    NN products of <= 64 columns then).  pad: floats between the rows of every window (A, B and C); a_off / b_off:
    floats by which the window of A / B starts off its 16-byte phase; kseg: the segmented-K layout of seg_layout();
    beta1: also run alpha = 1, beta = 1 with a bias"""

    def __init__(self, name, prec, ta, tb, M, N, K, route, route0=None, pad=4, a_off=0, b_off=0, kseg=0, beta1=False):
        self.name, self.prec, self.ta, self.tb, self.M, self.N, self.K = name, prec, bool(ta), bool(tb), M, N, K
        self.route, self.route0 = route, route0 or route
        self.pad, self.a_off, self.b_off, self.kseg, self.beta1 = pad, a_off, b_off, kseg, beta1

    def __repr__(self):
        return self.name

    def claimed(self, beta):
        return self.route0 if beta == 0 else self.route


GUARD = 2              # rows before and after every window
SEG_LDA, SEG_LDB = 32, 64


def layout(c):
    """Where the windows lie.  Every operand is a flat buffer; the dict gives its size in floats, the offset `start`
    of the pointer that is passed, the leading dimensions and segment strides of the call, and whether the pointers
    are 16-byte aligned (the buffers themselves are).  Plain windows: rows of width + pad floats, GUARD rows before
    and after, the window a_off / b_off floats into its first row.  Segmented K (the step-wise BLSTM's dWh =
    sum_b h[b, :-1]^T dz[b, 1:]): A = h is [segments, kseg + 1, 32] of which the product reads rows 0 .. kseg - 1 and
    columns 0 .. M - 1 of each segment (the other direction's half and the last row are not its business), B = dz is
    [segments, kseg + 1, 64] read from row 1 on: segments one row apart in both operands."""
    M, N, K = c.M, c.N, c.K
    L = {'ldc': N + c.pad, 'a_seg': 0, 'b_seg': 0}
    if c.kseg:
        assert c.ta and not c.tb and K % c.kseg == 0 and M <= SEG_LDA and N <= SEG_LDB
        rows = (K // c.kseg) * (c.kseg + 1) + 2 * GUARD
        L.update(lda=SEG_LDA, ldb=SEG_LDB, a_seg=(c.kseg + 1) * SEG_LDA, b_seg=(c.kseg + 1) * SEG_LDB,
                 a_size=rows * SEG_LDA, b_size=rows * SEG_LDB, a_start=GUARD * SEG_LDA, b_start=(GUARD + 1) * SEG_LDB)
    else:
        ar, ac = (K, M) if c.ta else (M, K)
        br, bc = (N, K) if c.tb else (K, N)
        L.update(lda=ac + c.pad, ldb=bc + c.pad)
        L.update(a_size=(ar + 2 * GUARD) * L['lda'] + 4, b_size=(br + 2 * GUARD) * L['ldb'] + 4,
                 a_start=GUARD * L['lda'] + c.a_off, b_start=GUARD * L['ldb'] + c.b_off)
    L.update(c_size=(M + 2 * GUARD) * L['ldc'], c_start=GUARD * L['ldc'])
    L['aligned'] = (L['a_start'] % 4 == 0, L['b_start'] % 4 == 0, L['c_start'] % 4 == 0)
    return L


def indices(c, L=None):
    """flat offsets (from the start of the buffer) of op(A)[m, k], op(B)[k, n] and C[m, n]: the addressing that
    include/nabu_hip.h states for nabu_gemm_f32"""
    L = L or layout(c)
    m, n, k = np.arange(c.M, dtype=np.int64), np.arange(c.N, dtype=np.int64), np.arange(c.K, dtype=np.int64)
    if c.kseg:
        ka = (k // c.kseg) * L['a_seg'] + (k % c.kseg) * L['lda']
        kb = (k // c.kseg) * L['b_seg'] + (k % c.kseg) * L['ldb']
    else:
        ka, kb = k * L['lda'], k * L['ldb']
    ia = L['a_start'] + (ka[None, :] + m[:, None] if c.ta else m[:, None] * L['lda'] + k[None, :])
    ib = L['b_start'] + (n[None, :] * L['ldb'] + k[:, None] if c.tb else kb[:, None] + n[None, :])
    ic = L['c_start'] + m[:, None] * L['ldc'] + n[None, :]
    return ia, ib, ic


def case_route(c, beta):
    L = layout(c)
    return route(c.prec, c.ta, c.tb, c.M, c.N, c.K, L['lda'], L['ldb'], L['ldc'], beta, c.kseg, L['a_seg'], L['b_seg'],
                 L['aligned'])


def _c(*a, **k):
    return Case(*a, **k)


T1 = 'tail[fast32 x1 + generic x1]'
T4 = 'tail[fast32 x4 + generic x1]'

CASES = [
    # fast32, one k-slice, the four transposes: an edge tile in M and in N each
    _c('fast32-NN', 'f32', 0, 0, 132, 68, 48, 'fast32 x1'),
    _c('fast32-TN', 'f32', 1, 0, 132, 68, 48, 'fast32 x1'),
    _c('fast32-NT', 'f32', 0, 1, 129, 72, 48, 'fast32 x1'),
    _c('fast32-TT', 'f32', 1, 1, 132, 69, 48, 'fast32 x1'),
    # fast32 with split-K and the reduce kernel
    _c('fast32-split-NN', 'f32', 0, 0, 132, 68, 1040, 'fast32 x4'),
    _c('fast32-split-TN', 'f32', 1, 0, 132, 260, 1040, 'fast32 x4'),
    # the generic kernel on shape grounds, four transposes (NN with rows off the 16-byte phase: odd pad)
    _c('generic-NN-oddpad', 'f32', 0, 0, 130, 70, 50, 'generic x1', pad=3),
    _c('generic-TN', 'f32', 1, 0, 130, 70, 50, 'generic x1'),
    _c('generic-NT', 'f32', 0, 1, 130, 70, 50, 'generic x1'),
    _c('generic-TT', 'f32', 1, 1, 130, 70, 50, 'generic x1'),
    # the generic kernel on alignment grounds: a fast32 shape whose A (B) starts one float into its buffer
    _c('generic-A-off', 'f32', 0, 0, 132, 68, 48, 'generic x1', a_off=1),
    _c('generic-B-off', 'f32', 0, 0, 132, 68, 48, 'generic x1', b_off=1),
    _c('generic-split-NN', 'f32', 0, 0, 131, 67, 1030, 'generic x4'),
    _c('generic-split-TN', 'f32', 1, 0, 131, 67, 1030, 'generic x4'),
    # K tail: after a one-slice head (bias once, beta once), after a split-K head and its reduce
    _c('tail-NN', 'f32', 0, 0, 132, 68, 88, T1, beta1=True),
    _c('tail-split-TN', 'f32', 1, 0, 132, 68, 1096, T4),
    _c('tail-split-NT', 'f32', 0, 1, 133, 68, 1096, T4),
    # smallk: one chunk, two chunks (28 + 24), the longest; its compositions; just below the rule
    _c('smallk-K8', 'f32', 0, 0, 2049, 132, 8, 'smallk'),
    _c('smallk-K52', 'f32', 0, 0, 2049, 132, 52, 'smallk'),
    _c('smallk-K96', 'f32', 0, 0, 2049, 132, 96, 'smallk'),
    _c('smallk-smallk', 'f32', 0, 0, 2049, 132, 72, 'tail[smallk + smallk]'),
    _c('smallk-generic', 'f32', 0, 0, 2048, 68, 100, 'tail[smallk + generic x1]'),
    _c('smallk-below', 'f32', 0, 0, 2047, 132, 96, 'fast32 x1'),
    # skinny: one chunk, MT = 2 with one row in the second tile, five chunks, just above the rule, narrow | skinny
    _c('skinny-1row', 'f32', 0, 0, 1, 32, 64, 'skinny x1', 'narrow', beta1=True),
    _c('skinny-33', 'f32', 0, 0, 33, 96, 192, 'skinny x3'),
    _c('skinny-64', 'f32', 0, 0, 64, 96, 320, 'skinny x5'),
    _c('skinny-above', 'f32', 0, 0, 65, 96, 320, 'fast32 x1'),
    _c('narrow-or-skinny', 'f32', 0, 0, 17, 64, 64, 'skinny x1', 'narrow', beta1=True),
    # the bf16 plane kernels
    _c('bf16-NN', 'bf16', 0, 0, 132, 68, 64, 'bf16 x1'),
    _c('bf16x3-NN', 'bf16x3', 0, 0, 132, 68, 64, 'bf16x3 x1'),
    _c('bf16x6-NN', 'bf16x6', 0, 0, 132, 68, 64, 'bf16x6 x1'),
    _c('bf16x3-TT', 'bf16x3', 1, 1, 132, 68, 96, 'bf16x3 x1'),
    _c('bf16x6-split-TN', 'bf16x6', 1, 0, 132, 260, 2048, 'bf16x6 x8'),
    # shapes the plane kernels refuse take the exact fp32 route of the same call; skinny whatever the precision
    _c('bf16-K48', 'bf16', 0, 0, 132, 68, 48, 'fast32 x1'),
    _c('bf16-M130', 'bf16', 0, 0, 130, 68, 64, 'fast32 x1'),
    _c('bf16-A-off', 'bf16', 0, 0, 132, 68, 64, 'generic x1', a_off=1),
    _c('bf16-skinny', 'bf16', 0, 0, 32, 96, 512, 'skinny x2'),
    # segmented K, the dWh product's layout
    _c('seg96-fast32', 'f32', 1, 0, 16, 64, 1152, 'fast32 x4', kseg=96),
    _c('seg96-bf16x6', 'bf16x6', 1, 0, 16, 64, 1152, 'bf16x6 x4', kseg=96),
    _c('seg13-fast32', 'f32', 1, 0, 16, 64, 1040, 'fast32 x4', kseg=13),      # every k-tile straddles a boundary
    _c('seg8-tail', 'f32', 1, 0, 16, 64, 200, T1, kseg=8),                    # the tail is exactly the last segment
    _c('seg5-generic', 'f32', 1, 0, 16, 64, 75, 'generic x1', kseg=5),        # a segment shorter than the tail
    # degenerate: C = beta * C + bias; nothing at all
    _c('K0', 'f32', 0, 0, 37, 21, 0, 'generic x1'),
    _c('M0', 'f32', 0, 0, 0, 20, 16, 'none'),
    _c('N0', 'f32', 0, 0, 20, 0, 16, 'none'),
]
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)

# every route the table must reach (tests/test_gemm_routes.py)
ROUTES = ['fast32 x1', 'fast32 x4', 'generic x1', 'generic x4', T1, T4, 'smallk', 'tail[smallk + smallk]',
          'tail[smallk + generic x1]', 'skinny x1', 'skinny x2', 'skinny x3', 'skinny x5', 'narrow', 'bf16 x1',
          'bf16x3 x1', 'bf16x6 x1', 'bf16x6 x4', 'bf16x6 x8', 'none']

# (alpha, beta, with a bias): beta = 0 runs on a window of C that holds NaN
EPILOGUES = [(1.0, 0.0, False), (-0.5, 2.0, True)]
EPILOGUE_BETA1 = (1.0, 1.0, True)


def epilogues(c):
    return EPILOGUES + ([EPILOGUE_BETA1] if c.beta1 else [])


# --------------------------------------------------------------------------------------------- operands and reference
def row_scale(n):
    return 2.0 ** ((7 * np.arange(n)) % 41 - 20)


def col_scale(n):
    return 2.0 ** ((5 * np.arange(n)) % 31 - 15)


_operands = {}


def scaled_operands(seed, M, N, K):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((M, K)) * row_scale(M)[:, None]).astype(np.float32)
    b = (rng.standard_normal((K, N)) * col_scale(N)[None, :]).astype(np.float32)
    c0 = (rng.standard_normal((M, N)) * col_scale(N)[None, :]).astype(np.float32)
    bias = (rng.standard_normal(N) * col_scale(N)).astype(np.float32)
    return a, b, c0, bias


def operands(c):
    """op(A) [M, K], op(B) [K, N], C0 [M, N], bias [N] in float32: made once per case, shared, never written to"""
    if c.name not in _operands:
        ops = scaled_operands(zlib.crc32(c.name.encode()), c.M, c.N, c.K)
        for x in ops:
            x.setflags(write=False)
        _operands[c.name] = ops
    return _operands[c.name]


def bound_of(prec, nround, alpha, beta, a, b, c0, bias):
    """(float64 result, componentwise bound) of alpha * a @ b + beta * c0 + bias for float32 a, b, c0, bias (bias may
    be None) evaluated in float32 with at most nround roundings per term, operands split into the planes of prec"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    prod, mag = a64 @ b64, abs(alpha) * (np.abs(a64) @ np.abs(b64))
    ref, rest = alpha * prod, np.zeros_like(prod)
    if beta != 0:
        ref = ref + beta * c0.astype(np.float64)
        rest = rest + abs(beta) * np.abs(c0.astype(np.float64))
    if bias is not None:
        ref = ref + bias.astype(np.float64)
        rest = rest + np.abs(bias.astype(np.float64))
    return ref, gamma(nround) * (mag + rest) + PLANE_TERM[prec] * mag


def reference(c, epilogue=EPILOGUES[1]):
    """(float64 result [M, N], componentwise bound [M, N]) of a case under (alpha, beta, with a bias)"""
    alpha, beta, with_bias = epilogue
    a, b, c0, bias = operands(c)
    r = case_route(c, beta)
    # the arithmetic of the kernels that run: the fp32 routes of a call that asked for planes are exact fp32
    prec = c.prec if r.startswith('bf16') else 'f32'
    return bound_of(prec, c.K + slices(r) + 3, alpha, beta, a, b, c0, bias if with_bias else None)


# ------------------------------------------------------------------------------------------------------ nabu_gemm2_f32
# (M, N, K1, K2): one chunk and no ticket path; chunk 256; chunk 64 with four tickets per column slice; K1 < K2
GEMM2_SHAPES = [(1, 32, 64, 0), (64, 96, 256, 256), (33, 64, 192, 64), (5, 32, 128, 320)]


def gemm2_chunk(K1, K2):
    """gemm_skinny.hip gemm_skinny_fused: the largest of 256 / 128 / 64 that divides K1 and K2"""
    for kc in (256, 128, 64):
        if K1 % kc == 0 and K2 % kc == 0:
            return kc
    return 0


def gemm2_reference(M, N, K1, K2, beta, with_bias=True):
    """operands of [A | A2] . [B ; B2] as ONE scaled pair a [M, K1 + K2], b [K1 + K2, N] (the caller cuts them at K1),
    c0, bias; the float64 result and its bound with S = (K1 + K2) / chunk slices"""
    a, b, c0, bias = scaled_operands(7919 * M + 31 * N + K1 + 3 * K2, M, N, K1 + K2)
    S = (K1 + K2) // gemm2_chunk(K1, K2)
    ref, bound = bound_of('f32', K1 + K2 + S + 3, 1.0, beta, a, b, c0, bias if with_bias else None)
    return (a, b, c0, bias), ref, bound
