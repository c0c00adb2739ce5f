"""The packed products (nabu_gemm_pk, csrc/gemm_pk.hip): a plane-exact restatement of what the kernel is meant to
compute, a restatement of its routing, a table of cases that reaches every instantiation and route, and the yardstick
the dense cases are held to.  Host code only (NumPy): tests/test_gemm_pk_cases.py holds all of it to its promises
without a device, tests/test_hip_gemm_pk_routes.py and tests/gemm_pk_routes_check.py run the cases on one.

THE RESTATEMENT.  The operands are held as the planes the pack kernels write (pack_ref / pack_ref_f16 below: the
layout and the split of include/nabu_hip.h, bit-tested against the device in tests/test_hip_gemm_pk.py).  In float64,

    planes = 2 (f16x3)   y = alpha inv_a[m] inv_b[n] sum_k (l_a h_b + h_a l_b + h_a h_b) + beta c0 + bias
    planes = 3 (bf16x6)  the same over l.h, h.l, m.m, m.h, h.m, h.h (inv = 1)
    planes = 1           the same over h.h alone

per batch entry, the columns >= n_split going to C2 under bias2.  What the arithmetic loses by design (the planes'
representation of x, the dropped l.l / m.l / l.m products) is IN y and is no error; what a device result may differ
from y by is what accumulating in float32 loses, and nothing else.

GRID CASES have operands on a small grid, so that every plane is non-zero, every plane product is a multiple of one
quantum q[m, n] and sum_k |products| < 2^24 q: every partial sum of any subset in any order is then a float32 number
and every float32 addition is exact — the device result is y bit for bit whatever the tile loop, the ring, the
split-K pass or the matrix instruction's internal order do (as long as the instruction adds exactly representable
partial sums exactly; LABNOTES.md section 35).  operands() proves the condition for every grid case and evaluates the
plane products in float32 forwards, backwards and in a random order against float64.

DENSE CASES have seeded normal operands, rows and columns scaled over many binary orders (the rule of
tests/gemm_routes.py).  judge() compares a result with y on every 32 x 32 window of the output (the MFMA tile):
e[w] = max over the window of |C - y| / T, T = |alpha| sum_k |a_k| |b_k| + |beta c0| + |bias|, against K of
tests/ctc_cases.py (4, the project's standing yardstick) times the largest e[w] of a float32 evaluation of the same
restatement on that case (one fused multiply-add per plane product and k, in order), plus 2 u.  K <= about 1000:
beyond that float32 accumulation hides a missing low-plane block and the grid cases take over."""
import collections
import zlib

import numpy as np

from tests import gemm_routes as G32
from tests.ctc_cases import K as YARD

U = 2.0 ** -24
FLOOR = 2 * U
PK_T = 256             # gemm_pk.hip: tile edge
PK_GM = 4              # row tiles per band
WIN = 32               # the MFMA tile
NCU = 256              # the device the table is designed for (MI355X): pk_cu_count()
KBS = {1: 3, 2: 1, 3: 1}              # k-blocks per stage
MIN_STAGES = {1: 24, 2: 48, 3: 24}    # nabu_gemm_pk / pk_fill: the shortest k-slice the policy cuts
# (plane of A, plane of B) of every plane product, in the order of the kernel's chains: smallest first
PRODUCTS = {1: [(0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]}


# ------------------------------------------------------------------------------------------- the packs, restated
def bf16_rne(x):
    """float32 array -> (uint16 bf16 bits, float32 value of the rounded number)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    return r.astype(np.uint16), (r << 16).astype(np.uint32).view(np.float32)


def split_planes(x, planes):
    out = []
    rest = np.ascontiguousarray(x, dtype=np.float32)
    for _ in range(planes):
        bits, val = bf16_rne(rest)
        out.append(bits)
        rest = (rest - val).astype(np.float32)
    return out, rest


def pack_ref(mat, planes, rows_pad, nkb):
    """mat [rows, K] float32 -> uint16 [nkb, planes, rows_pad, 16] in the layout of include/nabu_hip.h"""
    rows, K = mat.shape
    full = np.zeros((rows_pad, nkb * 16), np.float32)
    full[:rows, :K] = mat
    pl, rest = split_planes(full, planes)
    if planes == 3:
        assert not rest.any()                      # the three planes hold the fp32 value exactly
    out = np.zeros((nkb, planes, rows_pad, 16), np.uint16)
    swap = ((np.arange(rows_pad) >> 3) & 1).astype(bool)
    for p in range(planes):
        blk = pl[p].reshape(rows_pad, nkb, 2, 8).copy()
        blk[swap] = blk[swap][:, :, ::-1, :]
        out[:, p] = blk.reshape(rows_pad, nkb, 16).transpose(1, 0, 2)
    return out


def f16_scale_exp(amax):
    """exponent field -> (scale, inverse) as gemm_pk.hip derives them from the row maximum's bit pattern"""
    bits = np.ascontiguousarray(amax, dtype=np.float32).view(np.uint32)
    e = ((bits >> 23) & 0xFF).astype(np.int64)
    e = np.where((bits & 0x7FFFFFFF) == 0, 127, e)
    e = np.clip(e, 15, 253)
    return np.exp2(141.0 - e).astype(np.float32), np.exp2(e - 141.0).astype(np.float32)


def pack_ref_f16(mat, amax, rows_pad, nkb):
    """mat [rows, K] float32, amax [rows] -> uint16 [nkb, 2, rows_pad, 16]"""
    rows, K = mat.shape
    full = np.zeros((rows_pad, nkb * 16), np.float32)
    full[:rows, :K] = mat
    am = np.zeros(rows_pad, np.float32)
    am[:rows] = amax
    scale = f16_scale_exp(am)[0]
    xs = (full * scale[:, None]).astype(np.float32)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)).astype(np.float16)
    out = np.zeros((nkb, 2, rows_pad, 16), np.uint16)
    swap = ((np.arange(rows_pad) >> 3) & 1).astype(bool)
    for p, pl in enumerate((h, l)):
        blk = pl.view(np.uint16).reshape(rows_pad, nkb, 2, 8).copy()
        blk[swap] = blk[swap][:, :, ::-1, :]
        out[:, p] = blk.reshape(rows_pad, nkb, 16).transpose(1, 0, 2)
    return out, h, l, scale


def unpack_planes(packed, rows, f16):
    """the inverse of the layout: uint16 [nkb, planes, rows_pad, 16] -> float64 planes [planes][rows, nkb * 16], read
    from the very bits a device operand holds"""
    nkb, planes, rows_pad, _ = packed.shape
    swap = ((np.arange(rows_pad) >> 3) & 1).astype(bool)
    out = []
    for p in range(planes):
        blk = packed[:, p].transpose(1, 0, 2).reshape(rows_pad, nkb, 2, 8).copy()
        blk[swap] = blk[swap][:, :, ::-1, :]
        bits = np.ascontiguousarray(blk.reshape(rows_pad, nkb * 16)[:rows])
        val = bits.view(np.float16) if f16 else (bits.astype(np.uint32) << 16).view(np.float32)
        out.append(val.astype(np.float64))
    return out


# ---------------------------------------------------------------------------------------------- the routing, restated
def pk_rows_pad(rows):
    """gemm_pk.hip nabu_pk_rows_pad"""
    return (rows + PK_T - 1) // PK_T * PK_T


def pk_kblocks(K, planes):
    """gemm_pk.hip nabu_pk_kblocks: k-blocks of 16, rounded up to whole stages"""
    kbs, nkb = KBS[planes], (K + 15) // 16
    return (nkb + kbs - 1) // kbs * kbs


def pk_choose_split(ntiles, nkb, kbs, min_stages, ncu=NCU):
    """gemm_pk.hip pk_choose_split: (number of k-slices, k-blocks of a slice)"""
    nst = nkb // kbs
    best, best_eff = 1, 0.0
    maxs = max(1, min(32, nst // min_stages))
    for s in range(1, maxs + 1):
        per = (nst + s - 1) // s
        ns = (nst + per - 1) // per
        if ns != s:
            continue
        rounds = (ntiles * ns + ncu - 1) // ncu
        eff = float(ntiles) * nst / (float(rounds) * ncu * per) - 0.01 * (ns - 1)
        if eff > best_eff + 1e-9:
            best_eff, best = eff, ns
    per = (nst + best - 1) // best
    return (nst + per - 1) // per, per * kbs


def pk_forced_split(nkb, kbs, force):
    """gemm_pk.hip pk_fill under NABU_PK_SPLIT=force"""
    nst = nkb // kbs
    per = (nst + force - 1) // force
    return (nst + per - 1) // per, per * kbs


def pk_direct_rule(M, N, nkb, kb_per_split):
    """gemm_pk.hip nabu_gemm_pk, direct = 2: the direct chain when a workgroup's reduction is at most twice as long
    as the exact-fp32 kernel's would be (whose split is what nabu_gemm_ws_bytes tells: gemm_routes.ws_bytes)"""
    K = nkb * 16
    w32 = G32.ws_bytes(M, N, K)
    ns32 = w32 // (4 * M * N) if w32 else 1
    return kb_per_split * 16 <= 2 * (K // max(ns32, 1))


Route = collections.namedtuple('Route', 'kernel nsplit stages tiles_m tiles_n direct')


def route(c, split_env=-1, var_env=-1):
    """gemm_pk.hip pk_fill + nabu_gemm_pk: the instantiation gemm_pk_kernel<NP, VAR>, the number of k-slices (> 1: the
    reduce pass follows) and the stages of every slice.  split_env / var_env: NABU_PK_SPLIT / NABU_PK_VAR."""
    kbs, nkb = KBS[c.planes], pk_kblocks(c.K, c.planes)
    tm, tn = (c.M + PK_T - 1) // PK_T, (c.N + PK_T - 1) // PK_T
    ns, per = pk_choose_split(tm * tn * c.nbatch, nkb, kbs, MIN_STAGES[c.planes])
    if split_env > 0:
        ns, per = pk_forced_split(nkb, kbs, split_env)
    direct = c.planes == 2 and c.direct == 1
    if c.planes == 2 and c.direct == 2:
        direct = pk_direct_rule(c.M, c.N, nkb, per)
    var = var_env if var_env >= 0 else (0 if direct else 1)
    kernel = (1, 0) if c.planes == 1 else (c.planes, 0 if var == 0 else 1)
    stages = [(min(nkb, (s + 1) * per) - s * per) // kbs for s in range(ns)]
    return Route(kernel, ns, stages, tm, tn, direct)


def ws_bytes(c, split_env=-1):
    """gemm_pk.hip nabu_gemm_pk_ws_bytes"""
    r = route(c, split_env)
    return 4 * r.nsplit * c.nbatch * c.M * c.N if r.nsplit > 1 else 0


# ------------------------------------------------------------------------------------------------------------ the cases
class Case(object):
    """One call of nabu_gemm_pk.  kind: 'grid' (bit-exact) | 'dense' (judge()).  epi: (alpha, beta, with biases);
    beta == 0 starts from a C full of NaN.  n_split > 0: two destinations.  pad: floats between the rows of C and C2
    (ldc > N).  fill: how the operands are drawn — grid: 'f16' (+-1024 +- 0.25 scaled), 'f16sub' (2^-4 +- 2^-20: the l
    planes are fp16 subnormals), 'bf3' / 'bf1'; nnz > 0: every row of A keeps that many non-zero k.  dense: 'normal'
    (rows and columns scaled as in gemm_routes) | 'bounded' (A uniform in (-1, 1) under the a-priori bound 1).
    split / var: the child process (NABU_PK_SPLIT=3 / NABU_PK_VAR=0) runs the case too."""

    def __init__(self, name, kind, planes, M, N, K, epi, fill, direct=0, nbatch=1, n_split=0, pad=0, nnz=0, split=False,
                 var=False):
        self.name, self.kind, self.planes, self.M, self.N, self.K = name, kind, planes, M, N, K
        self.epi, self.fill, self.direct, self.nbatch, self.n_split, self.pad = epi, fill, direct, nbatch, n_split, pad
        self.nnz, self.split, self.var = nnz, split, var

    def __repr__(self):
        return self.name

    @property
    def widths(self):
        """columns of C and of C2"""
        return (self.n_split, self.N - self.n_split) if self.n_split else (self.N, 0)

    @property
    def ldc(self):
        return max(self.widths) + self.pad


E0 = (1.0, 0.0, False)          # plain: the kernel's `plain` epilogue, on a C that holds NaN
E1 = (-0.5, 2.0, True)          # alpha, beta and the biases
E2 = (1.0, 0.0, True)           # bias alone
E3 = (2.0, 0.0, False)          # alpha alone

CASES = [
    # ---- f16x3 on the grid: ring fill and drain (1, 2, 3, 4, 5, 7 stages), every edge in M and N
    Case('g2-st1-1x4', 'grid', 2, 1, 4, 16, E0, 'f16'),
    Case('g2-st2-31x60', 'grid', 2, 31, 60, 32, E1, 'f16', direct=2),
    Case('g2-st3-129x68', 'grid', 2, 129, 68, 40, E2, 'f16', direct=1, split=True, var=True),
    Case('g2-st4-256x256', 'grid', 2, 256, 256, 64, E1, 'f16'),
    Case('g2-st5-257x260', 'grid', 2, 257, 260, 80, E3, 'f16', direct=1, split=True),
    Case('g2-st7-two-dest', 'grid', 2, 300, 516, 112, E1, 'f16', n_split=256, pad=8, split=True),
    Case('g2-5x3-tiles', 'grid', 2, 1100, 516, 40, E0, 'f16', split=True),
    Case('g2-k1000', 'grid', 2, 300, 260, 1000, E1, 'f16'),
    Case('g2-split2', 'grid', 2, 257, 260, 1552, E1, 'f16', pad=4),            # 97 stages: slices of 49 and 48
    Case('g2-split3', 'grid', 2, 257, 260, 2320, E0, 'f16'),                   # 145 stages: 49, 49, 47
    Case('g2-k4000', 'grid', 2, 129, 68, 4000, E0, 'f16', direct=2),           # the longest exact reduction: one slice
    Case('g2-batch2', 'grid', 2, 129, 260, 48, E1, 'f16', nbatch=2, pad=4, split=True),
    Case('g2-subnormal-l', 'grid', 2, 129, 68, 80, E0, 'f16sub', split=True, var=True),
    # ---- bf16x6 on the grid: dense up to 48 terms, sparse rows of A beyond
    Case('g3-st1-31x4', 'grid', 3, 31, 4, 16, E1, 'bf3', var=True),
    Case('g3-st3-129x60', 'grid', 3, 129, 60, 40, E0, 'bf3', split=True, var=True),
    Case('g3-st7-sparse', 'grid', 3, 257, 68, 112, E1, 'bf3', nnz=40, split=True, var=True),
    Case('g3-two-dest', 'grid', 3, 300, 516, 48, E1, 'bf3', n_split=256, pad=4, var=True),
    Case('g3-split2-sparse', 'grid', 3, 257, 260, 784, E0, 'bf3', nnz=40, var=True),     # 49 stages: 25 and 24
    Case('g3-batch2', 'grid', 3, 31, 260, 32, E1, 'bf3', nbatch=2),
    # ---- one bf16 plane: stages of three k-blocks
    Case('g1-st1', 'grid', 1, 31, 60, 48, E1, 'bf1'),
    Case('g1-roundup', 'grid', 1, 129, 68, 100, E0, 'bf1', split=True),        # 7 k-blocks, rounded up to 9
    Case('g1-st5', 'grid', 1, 257, 260, 240, E1, 'bf1', split=True),
    Case('g1-split2', 'grid', 1, 257, 260, 2304, E0, 'bf1'),                   # 48 stages: 24 and 24
    # ---- dense, through judge()
    Case('d2-small', 'dense', 2, 129, 68, 40, E1, 'normal', split=True, var=True),
    Case('d2-k1000', 'dense', 2, 300, 260, 1000, E1, 'normal', split=True),
    Case('d2-k1000-direct', 'dense', 2, 300, 260, 1000, E0, 'normal', direct=1),
    Case('d2-rule-direct', 'dense', 2, 257, 260, 1000, E0, 'normal', direct=2),
    Case('d2-rule-promoted', 'dense', 2, 256, 256, 1024, E1, 'normal', direct=2),
    Case('d2-bounded', 'dense', 2, 300, 516, 336, E1, 'bounded', n_split=256, pad=4, nbatch=2),
    Case('d3-small', 'dense', 3, 31, 60, 40, E0, 'normal', split=True, var=True),
    Case('d3-k1000', 'dense', 3, 300, 260, 1000, E1, 'normal', var=True),
    Case('d1-k700', 'dense', 1, 257, 68, 700, E1, 'normal', split=True),
]
BY_NAME = collections.OrderedDict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)
SPLIT_ENV = 3          # the child's NABU_PK_SPLIT


def split_cases():
    return [c for c in CASES if c.split]


def var_cases():
    return [c for c in CASES if c.var]


# ------------------------------------------------------------------------------------------------------- the operands
Operands = collections.namedtuple('Operands', 'a b c0 bias bound_a')    # a [nbatch][M, K], b [nbatch][N, K], c0 [nbatch][M, N], bias [N]
Planes = collections.namedtuple('Planes', 'A B inv_a inv_b packed_a packed_b amax_a amax_b')
_cache = {}


def _signs(rng, shape):
    return rng.integers(0, 2, shape) * 2.0 - 1.0


def _grid_matrix(rng, fill, rows, K, k_scale, k_zero, nnz):
    """one operand on the grid, unscaled by its rows' powers of two"""
    if fill == 'f16':
        x = 1024.0 * _signs(rng, (rows, K)) + 0.25 * _signs(rng, (rows, K))
    elif fill == 'f16sub':
        x = 2.0 ** -4 * _signs(rng, (rows, K)) + 2.0 ** -20 * _signs(rng, (rows, K))
    elif fill == 'bf3':
        x = _signs(rng, (rows, K)) * (1.0 + 2.0 ** -9 * _signs(rng, (rows, K)) + 2.0 ** -18)
    else:
        x = _signs(rng, (rows, K)) * (1.0 + 0.25 * rng.integers(0, 4, (rows, K)) + 2.0 ** -12)
    if nnz:
        keep = np.zeros((rows, K), bool)
        for r in range(rows):
            keep[r, rng.choice(K, min(nnz, K), replace=False)] = True
        x = np.where(keep, x, 0.0)
    if fill.startswith('f16'):
        x[:, k_scale] = 2.0 ** 14          # fixes the row's scale, at a k where the other operand holds zero
        x[:, k_zero] = 0.0
    return x


def _grid_operands(c):
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    ea = ((3 * np.arange(c.M)) % 4 - 2).astype(np.float64)
    eb = ((5 * np.arange(c.N)) % 4 - 1).astype(np.float64)
    a = [(_grid_matrix(rng, c.fill, c.M, c.K, 1, c.K - 2, c.nnz) * np.exp2(ea)[:, None]).astype(np.float32)
         for _ in range(c.nbatch)]
    b = [(_grid_matrix(rng, c.fill, c.N, c.K, c.K - 2, 1, 0) * np.exp2(eb)[:, None]).astype(np.float32)
         for _ in range(c.nbatch)]
    return rng, a, b


def _lsb(x):
    """the lowest set bit of every element of a float64 array (inf where the element is 0)"""
    m, e = np.frexp(x)
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    with np.errstate(divide='ignore'):
        return np.where(mi == 0, np.inf, low * np.exp2(e.astype(np.float64) - 53))


def _quantum(A, B, pairs):
    """[M, N]: the coarsest power of two that divides every plane product that is kept"""
    la = [_lsb(P).min(axis=1) for P in A]
    lb = [_lsb(P).min(axis=1) for P in B]
    return np.min([la[x][:, None] * lb[y][None, :] for x, y in pairs], axis=0)


def exact_f32(x):
    return bool((np.asarray(x, np.float64).astype(np.float32).astype(np.float64) == x).all())


def planes_of(c, mats, bound=None):
    """[nbatch][rows, K] float32 -> per batch entry: float64 planes [planes][rows, nkb * 16], inverse row scales,
    the packed reference and (f16x3) the row maxima the device has to find"""
    nkb = pk_kblocks(c.K, c.planes)
    out = []
    for mat in mats:
        rows = mat.shape[0]
        if c.planes == 2:
            amax = np.full(rows, bound, np.float32) if bound is not None else np.abs(mat).max(axis=1)
            packed = pack_ref_f16(mat, amax, pk_rows_pad(rows), nkb)[0]
            inv = f16_scale_exp(amax)[1].astype(np.float64)
        else:
            amax, inv = None, np.ones(rows)
            packed = pack_ref(mat, c.planes, pk_rows_pad(rows), nkb)
        out.append((unpack_planes(packed, rows, c.planes == 2), inv, packed, amax))
    return out


def eval32(A, B, pairs, order='fwd', seed=0):
    """sum over k and over the plane products `pairs` of A[qa][:, k] B[qb][:, k]^T in float32: one multiply (exact: the
    planes have 11 or 8 significant bits) and one float32 addition per (k, pair), in the given order"""
    At = [np.ascontiguousarray(p.astype(np.float32).T) for p in A]
    Bt = [np.ascontiguousarray(p.astype(np.float32).T) for p in B]
    live = [[bool(At[qa][k].any() and Bt[qb][k].any()) for (qa, qb) in pairs] for k in range(At[0].shape[0])]
    steps = [(k, i) for k in range(At[0].shape[0]) for i in range(len(pairs)) if live[k][i]]
    if order == 'bwd':
        steps.reverse()
    elif order == 'rnd':
        steps = [steps[i] for i in np.random.default_rng(seed).permutation(len(steps))]
    acc = np.zeros((At[0].shape[1], Bt[0].shape[1]), np.float32)
    tmp = np.empty_like(acc)
    for k, i in steps:
        qa, qb = pairs[i]
        np.multiply(At[qa][k][:, None], Bt[qb][k][None, :], out=tmp)
        acc += tmp
    return acc


def plane_sum(A, B, pairs):
    """float64: sum over the plane products, and the same over magnitudes"""
    S = sum(A[qa] @ B[qb].T for qa, qb in pairs)
    return S


def _certify_grid(c, ops, pl):
    """the promises of a grid case, or an AssertionError: every plane non-zero; one quantum per output under which
    sum |products| + the epilogue's terms stay below 2^24; three float32 orders equal to float64 bit for bit"""
    alpha, beta, with_bias = c.epi
    pairs = PRODUCTS[c.planes]
    for i in range(c.nbatch):
        (A, inv_a, _, _), (B, inv_b, _, _) = pl[0][i], pl[1][i]
        for P in A + B:
            assert (np.abs(P).max(axis=1) > 0).all(), '%s: a row with an empty plane' % c.name
        q = _quantum(A, B, pairs)
        mag = sum(np.abs(A[x]) @ np.abs(B[y]).T for x, y in pairs)
        sc = abs(alpha) * inv_a[:, None] * inv_b[None, :]
        rest = (np.abs(ops.bias)[None, :] if with_bias else 0.0) + abs(beta) * np.abs(ops.c0[i])
        assert (sc * mag + rest < 2.0 ** 24 * sc * q).all(), '%s: partial sums leave the exact range' % c.name
        assert not np.mod(rest / (sc * q), 1.0).any(), '%s: epilogue terms off the quantum' % c.name
        S = plane_sum(A, B, pairs)
        if c.fill == 'f16sub':
            assert all(np.abs(P[1]).max() < 2.0 ** -14 for P in (A, B)), '%s: l planes are not subnormal' % c.name
        for order in ('fwd', 'bwd', 'rnd'):
            got = eval32(A, B, pairs, order, seed=i)
            assert np.array_equal(got.astype(np.float64), S), '%s: float32 order %s differs from float64' % (c.name, order)
        v = sc * S
        assert exact_f32(v) and exact_f32(S)
        if with_bias:
            v = v + ops.bias[None, :]
            assert exact_f32(v)
        if beta != 0:
            assert exact_f32(v + beta * ops.c0[i])


def operands(c):
    """(Operands, (planes of A per batch entry, planes of B per batch entry)): made once per case, shared, read-only.
    A grid case is certified here: one that fails is not in the table."""
    if c.name in _cache:
        return _cache[c.name]
    alpha, beta, with_bias = c.epi
    if c.kind == 'grid':
        rng, a, b = _grid_operands(c)
        bound = None
    else:
        rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        bounded = c.fill == 'bounded'
        rs = np.ones(c.M) if bounded else G32.row_scale(c.M)
        cs = G32.col_scale(c.N) * (0.1 if bounded else 1.0)
        a = [((rng.uniform(-1, 1, (c.M, c.K)) if bounded else rng.standard_normal((c.M, c.K))) * rs[:, None]).astype(np.float32)
             for _ in range(c.nbatch)]
        b = [(rng.standard_normal((c.N, c.K)) * cs[:, None]).astype(np.float32) for _ in range(c.nbatch)]
        bound = 1.0 if bounded else None
    pl = (planes_of(c, a, bound), planes_of(c, b))
    if c.kind == 'grid':
        # the epilogue's terms on the grid of the result: multiples of the coarsest quantum of their column (bias)
        # resp. of their element (c0)
        q = None
        for i in range(c.nbatch):
            (A, inv_a, _, _), (B, inv_b, _, _) = pl[0][i], pl[1][i]
            qi = abs(alpha) * inv_a[:, None] * inv_b[None, :] * _quantum(A, B, PRODUCTS[c.planes])
            q = qi if q is None else np.maximum(q, qi)
        bias = (rng.integers(-64, 65, c.N) * q.max(axis=0)).astype(np.float32)
        c0 = [(rng.integers(-64, 65, (c.M, c.N)) * q).astype(np.float32) for _ in range(c.nbatch)]
    else:
        mag = np.sqrt(c.K) * rs[:, None] * cs[None, :]
        bias = (rng.standard_normal(c.N) * cs * np.sqrt(c.K)).astype(np.float32)
        c0 = [(rng.standard_normal((c.M, c.N)) * mag).astype(np.float32) for _ in range(c.nbatch)]
    ops = Operands(a, b, c0, bias, bound)
    for x in a + b + c0 + [bias]:
        x.setflags(write=False)
    if c.kind == 'grid':
        _certify_grid(c, ops, pl)
    _cache[c.name] = (ops, pl)
    return _cache[c.name]


# -------------------------------------------------------------------------------------------- value, yardstick, judge
def epilogue64(c, ops, i, S, inv_a, inv_b):
    alpha, beta, with_bias = c.epi
    y = alpha * inv_a[:, None] * inv_b[None, :] * S
    if with_bias:
        y = y + ops.bias.astype(np.float64)[None, :]
    if beta != 0:
        y = y + beta * ops.c0[i].astype(np.float64)
    return y


def value(c, i=0, drop=None):
    """float64 [M, N]: what batch entry i of the case is meant to hold (columns >= n_split: C2).  drop: a function
    (A, B, pairs) -> float64 [M, N] subtracted from the plane sum (the mutations of tests/test_gemm_pk_cases.py)."""
    ops, pl = operands(c)
    (A, inv_a, _, _), (B, inv_b, _, _) = pl[0][i], pl[1][i]
    S = plane_sum(A, B, PRODUCTS[c.planes])
    if drop is not None:
        S = S - drop(A, B, PRODUCTS[c.planes])
    return epilogue64(c, ops, i, S, inv_a, inv_b)


def magnitude(c, i=0):
    """T of judge(): |alpha| sum_k |a_k| |b_k| + |beta c0| + |bias|, a_k and b_k the values the planes hold"""
    ops, pl = operands(c)
    alpha, beta, with_bias = c.epi
    (A, inv_a, _, _), (B, inv_b, _, _) = pl[0][i], pl[1][i]
    T = abs(alpha) * inv_a[:, None] * inv_b[None, :] * (np.abs(sum(A)) @ np.abs(sum(B)).T)
    if with_bias:
        T = T + np.abs(ops.bias.astype(np.float64))[None, :]
    if beta != 0:
        T = T + abs(beta) * np.abs(ops.c0[i].astype(np.float64))
    return T


def value32(c, i=0):
    """the same restatement evaluated in float32: the plane products one fused multiply-add per (k, product) in order,
    then the epilogue's operations one rounding each"""
    ops, pl = operands(c)
    alpha, beta, with_bias = c.epi
    (A, inv_a, _, _), (B, inv_b, _, _) = pl[0][i], pl[1][i]
    v = eval32(A, B, PRODUCTS[c.planes])
    v = v * (inv_a.astype(np.float32)[:, None] * inv_b.astype(np.float32)[None, :]) * np.float32(alpha)
    if with_bias:
        v = v + ops.bias[None, :]
    if beta != 0:
        v = v + np.float32(beta) * ops.c0[i]
    return v.astype(np.float32)


def window_max(e):
    """[M, N] -> the maximum over every 32 x 32 window (the last ones partial)"""
    M, N = e.shape
    mw, nw = (M + WIN - 1) // WIN, (N + WIN - 1) // WIN
    full = np.zeros((mw * WIN, nw * WIN))
    full[:M, :N] = e
    return full.reshape(mw, WIN, nw, WIN).max(axis=(1, 3))


def window_errors(c, got, i=0):
    y, T = value(c, i), magnitude(c, i)
    d = np.abs(np.asarray(got, np.float64) - y)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(T > 0, d / T, np.where(d > 0, np.inf, 0.0))
    e = np.where(np.isfinite(np.asarray(got, np.float64)), e, np.inf)
    return window_max(e)


_yard = {}


def yardstick(c, i=0):
    """the largest window error of the float32 evaluation on this case and batch entry"""
    if (c.name, i) not in _yard:
        _yard[(c.name, i)] = float(window_errors(c, value32(c, i), i).max())
    return _yard[(c.name, i)]


Verdict = collections.namedtuple('Verdict', 'ok worst allowance yard ratio where')


def judge(c, got, i=0):
    """got [M, N] against value(c, i): every window's e[w] <= K * yardstick + 2 u.  ratio = worst e[w] / yardstick:
    what LABNOTES.md reports against the allowance of K = 4."""
    ew = window_errors(c, got, i)
    yard = yardstick(c, i)
    allowance = YARD * yard + FLOOR
    worst = float(ew.max())
    where = tuple(int(x) for x in np.unravel_index(int(ew.argmax()), ew.shape))
    return Verdict(bool(worst <= allowance), worst, allowance, yard, worst / yard if yard > 0 else float('inf'), where)
