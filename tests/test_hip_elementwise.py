"""GPU: the small end of include/nabu_hip.h — pad_time / unpad_time, swap01, mask_time, ceil_div, clip, relu, axpy, sum,
colsum, the whole-utterance layer norm and the Speller's LSTM cell — each called directly (nabu_amd.ops) at its edge
shapes and at ONE size just above the launch cap of its grid-stride kernel (2048 workgroups x 256 threads = 524 288
work items: a float4 for pad_time and clip, an element for the others), against NumPy in float64 (the oracle's
functions and tests/elementwise_ref.py).

Every output element is compared, never a maximum normalised by the tensor's largest value.  Outputs the caller
allocates are filled with NaN first; for the wrappers that allocate their own output one case per op calls the entry
point on a 16-byte-aligned view in the middle of a NaN-filled buffer and looks at the words on both sides.

Three kinds of expectation:
* data movement (pad, unpad, swap01, mask_time, pyramid_stack): bit-exact on inputs holding -0.0, denormals, +-inf and
  NaN payloads, compared as uint32;
* exact arithmetic (ceil_div, clip, relu, relu_bwd: to the bit; axpy: the float64 value rounded, one ulp for the
  double rounding);
* rounded arithmetic: sum and colsum within the bound their summation shape gives (stated at the test); layer norm and
  the cell within RATIO x e32, where e32 is the max error of the float32 evaluation of the restatement against float64
  on the same inputs (the method of tests/test_hip_features.py), per output tensor of each case.

Measured on an MI355X (pytest -s prints them; LABNOTES.md section 26).  The cell: worst device error / e32 3.76 (h_new
of the one-unit case, 4.06e-8 against 1.08e-8), at most 2.59 on the larger shapes, so its bound stays at 4: the
__expf of sigmoidf_ / tanhf_ (common.h, "abs error ~1e-7") does not show at this level.  The layer norm: at most 3.01
(the mean of the 2 x 300 x 40 case) except for the row at mean 1000, whose mean is off by 1.07e-4 against the float32
evaluation's 1.54e-5 (ratio 6.91), and y, dx and dgamma with it (6.85, 7.07, 6.87).  The reason is in the kernel's
text: layer_norm_fwd_kernel forms the mean as ONE float32 sum of the row (256 chains, an 8-level tree, s / N).  The
12 000 elements sum to 1.2e7, where one ulp is 1.0, i.e. 8.3e-5 of the mean: the device's sum is 1.28 ulp from the
exact one, NumPy's pairwise sum happens to land 0.18 ulp from it.  The variance is not touched by this (rstd: ratio
0.66 — the second pass over x - mean is what the case is there to prove).  That case's bound is therefore twice its
measured ratio; every other case keeps 4."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from tests import elementwise_ref as R

pytestmark = pytest.mark.gpu

CAP = 2048 * 256                    # work items of one launch of a grid-stride kernel
LN_RATIO = 4.0                      # device error <= RATIO * e32: the allowance for another summation order
LN_RATIO_MEAN_1000 = 2 * 7.07       # the row at mean 1000 only: twice the measured ratio (the module's docstring says why)
CELL_RATIO = 4.0
GUARD = 64                          # floats on each side of a guarded output (256 bytes: the view stays 16-byte aligned)
NAN = float('nan')

# -0.0, the smallest and the largest denormal of either sign, +-inf, quiet NaNs with payloads of either sign
SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x807fffff, 0x007fffff, 0x7f800000, 0xff800000, 0x7fc00001,
                         0xffc12345, 0x7fffffff, 0x00000000], np.uint32)


def _hip():
    from nabu_amd import _hip, ops
    return _hip, ops


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device='cuda')


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def with_specials(shape, seed, every=7, scale=1.0):
    """float32 normals with every `every`-th element one of SPECIAL_BITS in turn"""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal(int(np.prod(shape)))).astype(np.float32)
    at = np.arange(seed % every, x.size, every)
    x.view(np.uint32)[at] = SPECIAL_BITS[np.arange(at.size) % SPECIAL_BITS.size]
    return x.reshape(shape)


def same_bits(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, '%d of %d words differ, the first at %d: %08x for %08x' % (
        bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def guarded(n):
    """(buffer, view): n floats in the middle of a NaN-filled buffer"""
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device='cuda')
    view = buf[GUARD:GUARD + n]
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(*pairs):
    for buf, view in pairs:
        b = host(buf)
        n = view.numel()
        assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + n:]).all(), 'a word outside the output was written'


def call(name, *args):
    _h, _ = _hip()
    _h.check(getattr(_h.lib(), name)(*(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args), _h.stream()),
             name)


def ordered(a):
    """float32 -> int64 that counts representable numbers (ulp distance = difference)"""
    i = bits(a).astype(np.int64)
    return np.where(i & 0x80000000, -(i & 0x7fffffff), i)


# ------------------------------------------------------------------------------------------ pure data movement

PAD_SHAPES = [(1, 1, 1, 4), (3, 7, 8, 8), (2, 5, 9, 4), (5, 33, 36, 1024), (4, 1000, 1002, 528)]


@pytest.mark.parametrize('B,T,Tp,F', PAD_SHAPES)
def test_pad_time_and_unpad_time_move_every_word_unchanged(B, T, Tp, F):
    _, ops = _hip()
    if (B, T, Tp, F) == PAD_SHAPES[-1]:
        assert B * Tp * (F // 4) == 529056 > CAP and B * T * (F // 4) > CAP      # both directions stride the grid
    x = with_specials((B, T, F), B + T)
    want = np.zeros((B, Tp, F), np.float32)
    want[:, :T] = x
    y = ops.pad_time(dev(x), Tp)
    same_bits(host(y), want)                                    # (padded frames: exact +0)
    same_bits(host(ops.unpad_time(y, T)), x)
    full = with_specials((B, Tp, F), B + Tp, every=5)           # unpad drops frames whatever they hold
    same_bits(host(ops.unpad_time(dev(full), T)), full[:, :T])


@pytest.mark.parametrize('B,T,Tp,F', [(3, 7, 8, 8), (4, 1000, 1002, 528)])
def test_pad_time_and_unpad_time_write_nothing_outside_their_output(B, T, Tp, F):
    x = with_specials((B, T, F), 3)
    want = np.zeros((B, Tp, F), np.float32)
    want[:, :T] = x
    ybuf, y = guarded(B * Tp * F)
    call('nabu_pad_time_f32', B, T, Tp, F, dev(x), y)
    same_bits(host(y).reshape(B, Tp, F), want)
    xbuf, back = guarded(B * T * F)
    call('nabu_unpad_time_f32', B, T, Tp, F, y, back)
    same_bits(host(back).reshape(B, T, F), x)
    guards_intact((ybuf, y), (xbuf, back))


def test_pad_time_refuses_a_feature_width_that_is_no_multiple_of_four_and_a_shorter_target():
    _h, ops = _hip()
    with pytest.raises(_h.NabuHipError):
        ops.pad_time(torch.zeros((2, 3, 6), device='cuda'), 4)
    with pytest.raises(_h.NabuHipError):
        ops.unpad_time(torch.zeros((2, 4, 6), device='cuda'), 3)
    with pytest.raises(_h.NabuHipError):
        ops.pad_time(torch.zeros((2, 3, 8), device='cuda'), 2)          # Tp < T
    with pytest.raises(_h.NabuHipError):
        ops.unpad_time(torch.zeros((2, 3, 8), device='cuda'), 4)        # T > Tp


SWAP_SHAPES = [(1, 1, 1), (7, 3, 5), (33, 17, 12), (40, 64, 260)]


@pytest.mark.parametrize('L,B,F', SWAP_SHAPES)
def test_swap01_is_swapaxes_and_its_own_inverse(L, B, F):
    _, ops = _hip()
    if (L, B, F) == SWAP_SHAPES[-1]:
        assert L * B * F > CAP
    x = with_specials((L, B, F), L + B)
    y = ops.swap01(dev(x))
    assert tuple(y.shape) == (B, L, F)
    same_bits(host(y), np.swapaxes(x, 0, 1))
    same_bits(host(ops.swap01(y)), x)


@pytest.mark.parametrize('L,B,F', [(7, 3, 5), (40, 64, 260)])
def test_swap01_writes_nothing_outside_its_output(L, B, F):
    x = with_specials((L, B, F), 5)
    buf, y = guarded(L * B * F)
    call('nabu_swap01_f32', L, B, F, dev(x), y)
    same_bits(host(y).reshape(B, L, F), np.swapaxes(x, 0, 1))
    guards_intact((buf, y))


@pytest.mark.parametrize('B,L,F', [(5, 9, 1), (5, 9, 5), (5, 9, 64), (5, 411, 257)])
def test_mask_time_zeroes_exactly_the_frames_past_each_length(B, L, F):
    _, ops = _hip()
    if L > 9:
        assert B * L * F > CAP
    lens = np.array([0, 1, L // 2, L + 3, L], np.int32)         # L + 3: nothing is masked for that row
    x = with_specials((B, L, F), F, every=3)
    want = x.copy()
    for b in range(B):
        want[b, lens[b]:] = 0.0
    masked = x[np.arange(L)[None, :] >= lens[:, None]]
    assert np.isnan(masked).any() and np.isinf(masked).any()    # NaN and inf inside the masked region too
    y = dev(x)
    assert ops.mask_time_(y, dev(lens)) is y
    same_bits(host(y), want)                                    # masked: exact +0; kept: bit-identical


@pytest.mark.parametrize('n', [1, 255, 256, 257, 70000])
def test_ceil_div_i32_is_exact(n):
    _, ops = _hip()
    rng = np.random.default_rng(n)
    for d in (1, 2, 3, 7):
        x = rng.integers(0, 2 ** 30 + 1, n).astype(np.int32)
        edge = np.array([0, 1, d - 1, d, d + 1, 2 ** 30, 2 ** 30 - 1, 2 * d, 2 * d + 1], np.int32)
        at = (np.arange(edge.size) * 29) % n
        x[at] = edge[:n] if n < edge.size else edge
        got = host(ops.ceil_div_i32(dev(x), d))
        want = -(-x.astype(np.int64) // d)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, d)


@pytest.mark.parametrize('numsteps', [2, 3])
@pytest.mark.parametrize('T', [1, 7, 8, 9])
def test_pyramid_stack_outputs_lengths_and_gradient_are_exact(T, numsteps):
    """the pad / ceil_div / unpad seam of components/ops.pyramid_stack under a tape, against the oracle: the stacked
    frames, both copies of the stacked lengths and the gradient handed back"""
    from nabu_amd.autodiff import Tape, SeqLen, record
    from nabu_amd.neuralnetworks.components import ops as cops
    B, F = 4, 8
    lens = np.array([T, 1, max(1, T - 1), (T + 1) // 2], np.int32)
    x = with_specials((B, T, F), T + numsteps, every=5)
    want, want_len = O.pyramid_stack_fwd(x, lens, numsteps)
    Tq = want.shape[1]
    dout = with_specials((B, Tq, numsteps * F), T, every=4)
    got = {}

    def capture(g):
        got['dx'] = g
        return [None]
    leaf, xd, root = dev(x), dev(x), torch.zeros(1, device='cuda')
    with Tape() as tape:
        record([leaf], [xd], capture)
        out, out_len = cops.pyramid_stack(xd, SeqLen(lens, torch.device('cuda')), numsteps)
        record([out], [root], lambda g: [dev(dout)])
    tape.backward(root)
    assert tuple(out.shape) == want.shape
    same_bits(host(out), want)
    assert out_len.host.dtype == np.int32 and np.array_equal(out_len.host, want_len)
    assert out_len.dev.dtype == torch.int32 and np.array_equal(host(out_len.dev), want_len)
    same_bits(host(got['dx']).reshape(B, T, F), O.pyramid_stack_bwd(dout, T, numsteps))


# ------------------------------------------------------------------------------------------ exact arithmetic

SIZES = [1, 3, 4, 5, 1023]


@pytest.mark.parametrize('bound', [1.0, 0.25])
@pytest.mark.parametrize('n', SIZES + [4 * CAP + 5])
def test_clip_is_numpy_clip_to_the_bit_and_keeps_nan(n, bound):
    _, ops = _hip()
    x = with_specials((n,), n, every=3, scale=2 * bound)
    x[-1] = -3 * bound                                          # the scalar tail has something to clip at every size
    if n > 100:
        assert np.isnan(x).any() and np.isinf(x).any()
    g = dev(x)
    assert ops.clip_(g, bound) is g
    got = host(g)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan)                   # NaN stays NaN, nothing else becomes one
    with np.errstate(invalid='ignore'):
        want = np.clip(x, np.float32(-bound), np.float32(bound))
    same_bits(np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, want).astype(np.float32))
    same_bits(np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, R.clip(x, bound, np.float32)))
    assert (got[np.isposinf(x)] == bound).all() and (got[np.isneginf(x)] == -bound).all()


def _relu_want(x):
    """positive inputs unchanged, everything else +0 (a NaN is checked apart)"""
    with np.errstate(invalid='ignore'):
        return np.where(x > 0, x, np.float32(0)).astype(np.float32)


@pytest.mark.parametrize('n', SIZES + [CAP + 257])
def test_relu_and_relu_bwd_to_the_bit_and_nan_stays_nan(n):
    _, ops = _hip()
    x = with_specials((n,), n + 1, every=3)
    y = ops.relu(dev(x))
    got = host(y)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan), 'relu: a NaN input must come out as NaN'
    same_bits(np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, _relu_want(x)).astype(np.float32))
    assert np.array_equal(np.where(nan, 0, got), np.where(nan, 0, O.relu_fwd(x.astype(np.float64))))
    with np.errstate(invalid='ignore'):
        assert not bits(got[(x <= 0) & ~nan]).any()             # negatives, -inf and +-0.0: exact +0
    assert (got[np.isposinf(x)] == np.inf).all()
    dy = with_specials((n,), n + 2, every=4)
    dx = host(ops.relu_bwd(y, dev(dy)))
    with np.errstate(invalid='ignore'):
        want = np.where(got > 0, dy, np.float32(0)).astype(np.float32)      # (y NaN: not > 0)
    same_bits(dx, want)


def test_relu_and_relu_bwd_write_nothing_outside_their_output():
    n = CAP + 257
    x, dy = with_specials((n,), 9, every=3), with_specials((n,), 10, every=4)
    ybuf, y = guarded(n)
    call('nabu_relu_f32', n, dev(x), y)
    dbuf, dx = guarded(n)
    call('nabu_relu_bwd_f32', n, y, dev(dy), dx)
    got = host(y)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan)
    same_bits(np.where(nan, 0, got).astype(np.float32), np.where(nan, 0, _relu_want(x)).astype(np.float32))
    with np.errstate(invalid='ignore'):
        same_bits(host(dx), np.where(got > 0, dy, np.float32(0)).astype(np.float32))
    guards_intact((ybuf, y), (dbuf, dx))


@pytest.mark.parametrize('F', [64, 10])
def test_relu_then_layer_norm_of_a_row_with_a_nan_is_not_finite(F):
    """a diverged pre-activation stays visible behind relu + layer norm: on the fused kernel (nabu_rows_relu_ln_fwd,
    F % 4 == 0) and on the path the DNN encoder composes where the kernel does not take F (relu + layer_norm_fwd);
    the other rows are what they are without the NaN, bit for bit"""
    _, ops = _hip()
    rng = np.random.default_rng(F)
    N, bad = 5, 2
    z = rng.standard_normal((N, F)).astype(np.float32)
    clean = z.copy()
    z[bad, 7] = NAN
    gamma, beta = dev(1 + 0.1 * rng.standard_normal(F).astype(np.float32)), dev(0.1 * rng.standard_normal(F).astype(np.float32))

    def run(rows):
        fwd = ops.rows_relu_ln_fwd(dev(rows), gamma, beta)
        assert (fwd is None) == (F % 4 != 0)
        if fwd is None:
            fwd = ops.layer_norm_fwd(ops.relu(dev(rows)), gamma, beta)
        return [host(t) for t in fwd]
    y, mean, rstd = run(z)
    y0, mean0, rstd0 = run(clean)
    assert np.isfinite(y0).all()
    assert not np.isfinite(y[bad]).any(), 'the row with a NaN came out finite'
    assert not np.isfinite(mean[bad]) and not np.isfinite(rstd[bad])
    ok = np.arange(N) != bad
    same_bits(y[ok], y0[ok])
    same_bits(mean[ok], mean0[ok])
    same_bits(rstd[ok], rstd0[ok])


@pytest.mark.parametrize('n', SIZES + [CAP + 257])
def test_axpy_is_one_fused_multiply_add(n):
    """y = fma(a, x, y): the float64 value a x + y rounded to float32, one ulp allowed for the double rounding"""
    _, ops = _hip()
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    y0 = rng.standard_normal(n).astype(np.float32)
    y0[::5] = -x[::5]                                           # cancellation for a = 1
    for a in (1.0, -0.5, 0.0):
        y = dev(y0)
        assert ops.axpy_(y, dev(x), a) is y
        want = (a * x.astype(np.float64) + y0.astype(np.float64)).astype(np.float32)
        ulps = np.abs(ordered(host(y)) - ordered(want))
        assert ulps.max() <= 1, (n, a, int(ulps.max()), int(ulps.argmax()))
        if a == 0.0:
            same_bits(host(y), y0)


# ------------------------------------------------------------------------------------------ rounded arithmetic

@pytest.mark.parametrize('scale', [1.0, 1.0 / 32])
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 100003])
def test_sum_within_the_bound_of_its_summation_shape(n, scale):
    """one workgroup: a serial chain of ceil(n / 256) additions per thread, then an 8-level tree, then the scale:
    |error| <= (ceil(n / 256) + 8) 2^-24 |scale| sum |x|.  The float32 restatement of that shape is the kernel's own
    sum (IEEE additions in a fixed order), so it is also compared bit for bit."""
    _, ops = _hip()
    x = (np.random.default_rng(n).standard_normal(n) + 0.25).astype(np.float32)
    xd = dev(x) if n else torch.empty(0, dtype=torch.float32, device='cuda')
    out = ops.sum_(xd, scale)
    got = host(out)
    assert got.shape == (1,) and got.dtype == np.float32
    same_bits(got, host(ops.sum_(xd, scale)))                   # two calls: identical bits
    ref = R.sum_tree(x, scale)
    bound = (-(-n // 256) + 8) * 2.0 ** -24 * abs(scale) * np.abs(x.astype(np.float64)).sum()
    err = abs(float(got[0]) - ref)
    print('sum n %d scale %g: error %.3g, bound %.3g' % (n, scale, err, bound))
    assert err <= bound
    if n == 0:
        assert got[0] == 0 and not np.signbit(got[0])
    same_bits(got, np.array([R.sum_tree(x, scale, np.float32)], np.float32))


def _colsum(a, out, beta):
    """ops.colsum for a contiguous matrix; a column window of a wider one (lda > N) or an empty one (whose torch
    pointer is null) reaches the entry point with its own pointer, as ops.colsum would pass it"""
    _h, ops = _hip()
    M, N = a.shape
    if M and a.is_contiguous():
        return ops.colsum(a, out, beta)
    lib = _h.lib()
    nbytes = lib.nabu_colsum_ws_bytes(M, N)
    ws = _h.Workspace.get(nbytes, out.device, 'gemm')
    base = a.data_ptr() if M else out.data_ptr()                # M = 0: any non-null pointer, nothing is read
    _h.check(lib.nabu_colsum_f32(M, N, base, a.stride(0) if M else N, beta, out.data_ptr(), ws.data_ptr(), nbytes,
                                 _h.stream()), 'nabu_colsum_f32')
    return out


@pytest.mark.parametrize('N', [1, 63, 64, 65, 300])
@pytest.mark.parametrize('M', [0, 1, 511, 512, 513, 1500])
def test_colsum_of_a_column_window_within_the_bound_of_its_summation_shape(M, N):
    """stage 1: blocks of 512 rows, four chains of at most 128 rows per column and a two-level tree (128 + 2
    additions); stage 2: the `parts` block sums one after the other, then beta * out: per column
    |error| <= (128 + 3 + parts) 2^-24 sum |a[:, c]|  (+ one rounding of the result and of beta * out when beta != 0).
    The matrix is a window of a wider one whose other columns hold NaN; beta = 0 must not read `out`."""
    rng = np.random.default_rng(1000 * M + N)
    wide = np.full((M, N + 5), NAN, np.float32)
    a = (rng.standard_normal((M, N)) + 0.5).astype(np.float32)
    wide[:, 2:2 + N] = a
    wd = dev(wide) if M else torch.empty((0, N + 5), dtype=torch.float32, device='cuda')
    win = wd[:, 2:2 + N]
    assert win.stride(0) == N + 5
    a64 = a.astype(np.float64)
    ref, mag = a64.sum(0), np.abs(a64).sum(0)
    parts = -(-M // 512)
    bound = (128 + 3 + parts) * 2.0 ** -24 * mag
    out = torch.full((N,), NAN, dtype=torch.float32, device='cuda')
    got = host(_colsum(win, out, 0.0))
    err = np.abs(got - ref)
    print('colsum %d x %d: worst error / bound %.3f' % (M, N, (err / np.maximum(bound, 1e-300)).max() if M else 0.0))
    assert np.isfinite(got).all() and (err <= bound).all()
    if M == 0:
        assert not bits(got).any()                              # exact +0
    else:
        same_bits(host(_colsum(dev(a), torch.full((N,), NAN, dtype=torch.float32, device='cuda'), 0.0)), got)
    out0 = rng.standard_normal(N).astype(np.float32)
    got = host(_colsum(win, dev(out0), 0.5))
    ref5 = 0.5 * out0.astype(np.float64) + ref
    bound5 = bound + 2.0 ** -24 * (np.abs(ref5) + np.abs(0.5 * out0))
    assert (np.abs(got - ref5) <= bound5).all()
    if M == 0:
        same_bits(got, (0.5 * out0).astype(np.float32))         # beta * out


def _ratios(tag, triples, limit):
    """triples: (name, device, float64 reference, float32 evaluation); prints every ratio, then asserts them all"""
    bad = []
    worst = 0.0
    for name, got, ref, ref32 in triples:
        got, ref, ref32 = np.asarray(got), np.asarray(ref), np.asarray(ref32)
        assert got.shape == ref.shape == ref32.shape and got.dtype == np.float32 and ref32.dtype == np.float32, name
        assert np.isfinite(got).all(), name
        e32 = np.abs(ref32.astype(np.float64) - ref).max() if ref.size else 0.0
        err = np.abs(got.astype(np.float64) - ref).max() if ref.size else 0.0
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float('inf'))
        worst = max(worst, ratio)
        print('%s %s: device error %.3g, e32 %.3g, ratio %.2f' % (tag, name, err, e32, ratio))
        if not err <= limit * e32:
            bad.append((name, err, e32, ratio))
    print('%s: worst ratio %.2f' % (tag, worst))
    assert not bad, (tag, bad)


def _ln_case(name):
    rng = np.random.default_rng(len(name))
    shape = {'tiny': (1, 1, 4), 'odd': (3, 7, 10), 'long': (2, 300, 40), 'wide': (4, 1, 2048),
             'constant_row': (3, 7, 10), 'mean_1000': (2, 300, 40)}[name]
    x = rng.standard_normal(shape).astype(np.float32)
    if name == 'constant_row':
        x[1] = 3.0              # sums of threes are exact: mean 3, variance 0, rstd = 1 / sqrt(eps), y = beta
    if name == 'mean_1000':
        x[0] += 1000.0          # E[x^2] - E[x]^2 in single precision would lose the unit variance here
    F = shape[-1]
    gamma = (1 + 0.1 * rng.standard_normal(F)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(F)).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    return x, gamma, beta, dy


def _ln_ref(x, gamma, beta, dy, dtype, eps):
    x, gamma, beta, dy = (a.astype(dtype) for a in (x, gamma, beta, dy))
    y, cache = O.layer_norm_fwd(x, gamma, beta, dtype(eps))
    dx, dgamma, dbeta = O.layer_norm_bwd(dy, cache)
    mean = x.reshape(x.shape[0], -1).mean(1)
    return dict(y=y, mean=mean, rstd=cache[1], dx=dx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize('name', ['tiny', 'odd', 'long', 'wide', 'constant_row', 'mean_1000'])
def test_layer_norm_fwd_and_bwd_within_four_times_the_single_precision_error(name):
    """y, mean, rstd, dx and the dgamma / dbeta partials summed with colsum, each within LN_RATIO x e32.  Measured
    worst ratios: tiny 1.00, odd 2.69 (mean), long 3.01 (mean), wide 1.00, constant_row 1.84 (mean); mean_1000 7.07
    (dx; mean 6.91, y 6.85, dgamma 6.87, rstd 0.66, dbeta 0.34), the one-ulp rounding of the float32 row sum of 1.2e7
    (the module's docstring): that case alone is held to LN_RATIO_MEAN_1000, and its rstd to LN_RATIO all the same"""
    _, ops = _hip()
    eps = 1e-12
    x, gamma, beta, dy = _ln_case(name)
    ref = _ln_ref(x, gamma, beta, dy, np.float64, eps)
    with np.errstate(all='ignore'):
        ref32 = _ln_ref(x, gamma, beta, dy, np.float32, eps)
    xd, gd = dev(x), dev(gamma)
    y, mean, rstd = ops.layer_norm_fwd(xd, gd, dev(beta), eps)
    dx, dgp, dbp = ops.layer_norm_bwd(xd, gd, dev(dy), mean, rstd)
    F = x.shape[-1]
    dgamma = ops.colsum(dgp, torch.full((F,), NAN, dtype=torch.float32, device='cuda'))
    dbeta = ops.colsum(dbp, torch.full((F,), NAN, dtype=torch.float32, device='cuda'))
    got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if name == 'constant_row':
        assert ref['mean'][1] == 3.0 and abs(ref['rstd'][1] - 1 / np.sqrt(eps)) < 1e-3
        assert host(mean)[1] == 3.0
        same_bits(host(y)[1], np.broadcast_to(beta, x.shape[1:]).copy())        # y = beta, exactly
    if name == 'mean_1000':
        assert abs(ref['rstd'][0] - 1.0) < 0.05
    strict = ('rstd', 'dbeta') if name == 'mean_1000' else ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')
    loose = [k for k in ('y', 'mean', 'dx', 'dgamma') if k not in strict]
    _ratios('layer_norm ' + name, [(k, host(got[k]), ref[k], ref32[k]) for k in strict], LN_RATIO)
    if loose:
        _ratios('layer_norm ' + name, [(k, host(got[k]), ref[k], ref32[k]) for k in loose], LN_RATIO_MEAN_1000)


def test_layer_norm_writes_nothing_outside_its_outputs():
    B, T, F = 3, 7, 10
    x, gamma, beta, dy = _ln_case('odd')
    ref = _ln_ref(x, gamma, beta, dy, np.float64, 1e-12)
    ref32 = _ln_ref(x, gamma, beta, dy, np.float32, 1e-12)
    xd, gd = dev(x), dev(gamma)
    (yb, y), (mb, mean), (rb, rstd) = guarded(B * T * F), guarded(B), guarded(B)
    call('nabu_layer_norm_fwd', B, T * F, F, xd, gd, dev(beta), 1e-12, y, mean, rstd)
    (db, dx), (gb, dgp), (bb, dbp) = guarded(B * T * F), guarded(B * F), guarded(B * F)
    call('nabu_layer_norm_bwd', B, T * F, F, xd, gd, dev(dy), mean, rstd, dx, dgp, dbp)
    guards_intact((yb, y), (mb, mean), (rb, rstd), (db, dx), (gb, dgp), (bb, dbp))
    _ratios('layer_norm guarded', [('y', host(y).reshape(B, T, F), ref['y'], ref32['y']),
                                   ('mean', host(mean), ref['mean'], ref32['mean']),
                                   ('rstd', host(rstd), ref['rstd'], ref32['rstd']),
                                   ('dx', host(dx).reshape(B, T, F), ref['dx'], ref32['dx'])], LN_RATIO)
    assert np.isfinite(host(dgp)).all() and np.isfinite(host(dbp)).all()


CELL_LENS = (3, 2, 1, 5, 0)       # at step 2: one row each below, at and above its length (and two more)


def _cell_run(B, U, with_emb, with_dh2, bias_edit=None, steps=(0, 2, 3, 5)):
    """the cell's forward and backward kernels at every step of `steps` on NaN-filled outputs: frozen rows exact, live
    rows through _ratios; returns the last live step's device activations and their float32 evaluation"""
    _, ops = _hip()
    rng = np.random.default_rng(B * 1000 + U)
    C = 6
    f32 = lambda a: a.astype(np.float32)
    z, bias = f32(rng.standard_normal((B, 4 * U))), f32(rng.standard_normal(4 * U))
    if bias_edit is not None:
        bias_edit(bias)
    c_prev, h_prev = f32(rng.standard_normal((B, U))), f32(rng.uniform(-1, 1, (B, U)))
    emb, ids = (f32(rng.standard_normal((C, 4 * U))), rng.integers(0, C, B).astype(np.int32)) if with_emb else (None, None)
    dh, dc_in = f32(rng.standard_normal((B, U))), f32(rng.standard_normal((B, U)))
    dh2 = f32(rng.standard_normal((B, U))) if with_dh2 else None
    seq_len = np.array([CELL_LENS[b % len(CELL_LENS)] for b in range(B)], np.int32)
    lens_d = dev(seq_len)
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float32, device='cuda')
    opt = lambda a: None if a is None else dev(a)
    last = None
    for step in steps:
        live = step < seq_len
        acts, c_new, h_new = nan(B, 4 * U), nan(B, U), nan(B, U)
        ops.lstm_cell_fwd(step, lens_d, dev(z), dev(bias), opt(emb), opt(ids), dev(c_prev), dev(h_prev), acts, c_new, h_new)
        ref = R.lstm_cell_fwd(step, seq_len, z, bias, c_prev, h_prev, emb, ids)
        ref32 = R.lstm_cell_fwd(step, seq_len, z, bias, c_prev, h_prev, emb, ids, np.float32)
        # the backward kernel reads what a forward pass stored: the reference's, rounded — the same inputs for all three
        acts_in, c_in = f32(ref[0]), f32(ref[1])
        dz, dc_out = nan(B, 4 * U), nan(B, U)
        ops.lstm_cell_bwd(step, lens_d, dev(acts_in), dev(c_in), dev(c_prev), dev(dh), opt(dh2), dev(dc_in), dz, dc_out)
        bref = R.lstm_cell_bwd(step, seq_len, acts_in, c_in, c_prev, dh, dc_in, dh2)
        bref32 = R.lstm_cell_bwd(step, seq_len, acts_in, c_in, c_prev, dh, dc_in, dh2, np.float32)
        got = [host(t) for t in (acts, c_new, h_new, dz, dc_out)]
        for g in got:
            assert np.isfinite(g).all(), 'an output word was not written, or is not finite'
        dead = ~live
        same_bits(got[1][dead], c_prev[dead])                   # frozen rows: state copied,
        same_bits(got[2][dead], h_prev[dead])
        assert not bits(got[0][dead]).any() and not bits(got[3][dead]).any()        # activations and dz exact +0,
        same_bits(got[4][dead], dc_in[dead])                    # dc handed through
        if live.any():
            names = ('acts', 'c_new', 'h_new', 'dz', 'dc_out')
            _ratios('lstm_cell (%d, %d) emb %d dh2 %d step %d' % (B, U, with_emb, with_dh2, step),
                    [(n, g[live], r[live], r32[live]) for n, g, r, r32 in zip(names, got, ref + bref, ref32 + bref32)],
                    CELL_RATIO)
            last = (got[0][live], ref32[0][live])
    return last


@pytest.mark.parametrize('with_dh2', [False, True])
@pytest.mark.parametrize('with_emb', [False, True])
@pytest.mark.parametrize('B,U', [(1, 1), (5, 20), (33, 64), (64, 320)])
def test_lstm_cell_fwd_and_bwd_within_four_times_the_single_precision_error(B, U, with_emb, with_dh2):
    _cell_run(B, U, with_emb, with_dh2)


def test_lstm_cell_with_saturated_gates_is_finite_and_exact_where_single_precision_is():
    """biases of +-88 .. +-690 on ten units per gate (saturating_bias of tests/test_hip_recurrence_range.py):
    everything finite, and a gate the float32 evaluation puts at exactly 0, 1 or -1 is exactly that on the device"""
    from tests.test_hip_recurrence_range import saturating_bias
    U = 64
    acts, acts32 = _cell_run(33, U, True, True, bias_edit=lambda b: saturating_bias(b, U), steps=(0,))
    exact = np.isin(acts32, (0.0, 1.0, -1.0))
    assert exact.sum() >= 20 * acts.shape[0]
    assert np.array_equal(acts[exact], acts32[exact])
