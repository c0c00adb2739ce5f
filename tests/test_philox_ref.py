"""CPU tests of the host Philox4x32-10 reference (oracle/philox.py) that the GPU
sampling tests (tests/test_hip_sampling.py) compare the kernels' draws with."""
import numpy as np
import pytest

from oracle import philox as P

# Random123's known-answer vectors for philox4x32-10 (kat_vectors: counter, key -> output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize('ctr,key,out', KAT)
def test_philox_known_answers(ctr, key, out):
    got = P.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == list(out)


def test_philox_vectorised_matches_one_at_a_time():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (37, 4), dtype=np.uint64).astype(np.uint32)
    key = np.array([0x12345678, 0x9abcdef0], np.uint32)
    many = P.philox4x32_10(ctr, key)
    for i in range(len(ctr)):
        np.testing.assert_array_equal(many[i], P.philox4x32_10(ctr[i], key))


def test_u01_is_the_top_24_bits():
    x = np.array([0, 255, 256, 0xffffffff, 0x80000000], np.uint32)
    np.testing.assert_array_equal(P.u01(x), [0.0, 0.0, 2.0 ** -24, 1 - 2.0 ** -24, 0.5])
    assert np.all(P.u01(x).astype(np.float32) == P.u01(x))          # exact in float32


def test_sample_words_counter_and_key_layout():
    """counter (row, 0, offset_lo, offset_hi), key (seed_lo, seed_hi)"""
    seed, offset = (7 << 32) | 11, (3 << 32) | 1000003
    x, y = P.sample_words(np.array([0, 5, 300]), seed, offset)
    for i, row in enumerate([0, 5, 300]):
        r = P.philox4x32_10(np.array([row, 0, 1000003, 3], np.uint32), np.array([11, 7], np.uint32))
        assert (x[i], y[i]) == (r[0], r[1])


def _scalar_draw(l, prob, seed, offset, teacher, row):
    x, y = P.sample_words(np.array([row]), seed, offset)
    if not P.u01(x)[0] < np.float32(prob):
        return teacher
    e = np.exp(np.asarray(l, np.float64) - max(l))
    target, acc = P.u01(y)[0] * e.sum(), 0.0
    for c, v in enumerate(e):
        acc += v
        if acc > target:
            return c
    return len(l) - 1


@pytest.mark.parametrize('C,prob', [(2, 1.0), (7, 0.3), (48, 1.0), (300, 0.5)])
def test_reference_draw_against_a_scalar_loop(C, prob):
    rng = np.random.default_rng(C)
    B = 64
    lg = rng.normal(size=(B, C)) * 2
    teacher = rng.integers(0, C, B)
    ids, sel, margin, bounds = P.reference_draw(lg, prob, 99, 1000003 * 4 + 2, teacher, row0=17)
    for b in range(B):
        assert ids[b] == _scalar_draw(lg[b], prob, 99, 1000003 * 4 + 2, teacher[b], b + 17)
        if sel[b]:
            assert bounds[b, 0] <= ids[b] <= bounds[b, 1]
            assert margin[b] >= 0
        else:
            assert ids[b] == teacher[b] and margin[b] == np.inf
    if prob == 1.0:
        assert sel.all()


def test_reference_draw_row0_shifts_the_counter():
    rng = np.random.default_rng(1)
    lg = rng.normal(size=(40, 9))
    t = np.zeros(40, np.int64)
    whole = P.reference_draw(lg, 0.7, 5, 123, t)[0]
    part = P.reference_draw(lg[16:], 0.7, 5, 123, t[16:], row0=16)[0]
    np.testing.assert_array_equal(whole[16:], part)


def test_reference_draw_statistics():
    """Bernoulli(prob) selection, then softmax(logits) frequencies"""
    B = 200000
    row = np.array([0.3, -1.0, 2.0, 0.0, 1.1], np.float64)
    ids, sel, _, _ = P.reference_draw(np.tile(row, (B, 1)), 0.25, 3, 8, np.full(B, -1))
    assert abs(sel.mean() - 0.25) < 5e-3
    sm = np.exp(row - row.max())
    sm /= sm.sum()
    freq = np.bincount(ids[sel], minlength=5) / sel.sum()
    assert np.abs(freq - sm).max() < 1e-2
    assert np.all(ids[~sel] == -1)


def test_reference_draw_boundary_margin():
    """two equal classes: u * total at the middle of the CDF has a margin of |u - 1/2|"""
    B = 1000
    ids, sel, margin, bounds = P.reference_draw(np.zeros((B, 2)), 1.0, 1, 2, np.zeros(B))
    x, y = P.sample_words(np.arange(B), 1, 2)
    u = P.u01(y)
    np.testing.assert_allclose(margin, np.minimum(np.abs(u - 0.5), 1 - u), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(ids, (u >= 0.5).astype(np.int64))
    near = np.abs(u - 0.5) <= 1e-5
    assert np.all(bounds[~near, 0] == bounds[~near, 1])


# ------------------------------------------------------------------------------------- dropout masks and noise


def test_dropout_scale_counter_key_and_lane_layout():
    """element e: lane e % 4 of Philox((e // 4 lo, hi, offset lo, hi), (seed lo, hi)), kept when u01 < keep"""
    seed, offset = (9 << 32) | 5, (1 << 32) | 77
    first = (3 << 32) * 4 + 8                           # a group index whose high word is 3
    s = P.dropout_scale(8, 0.5, seed, offset, first_elem=first)
    for j in range(8):
        g = (first + j) // 4
        r = P.philox4x32_10(np.array([g & 0xFFFFFFFF, g >> 32, 77, 1], np.uint32), np.array([5, 9], np.uint32))
        assert s[j] == (np.float32(2) if P.u01(r[j % 4]) < 0.5 else 0), j
    assert s.dtype == np.float32


def test_dropout_scale_keep_one_keeps_everything():
    s = P.dropout_scale(4099, 1.0, 123, (1 << 32) - 1)
    assert s.dtype == np.float32 and np.all(s == 1)


@pytest.mark.parametrize('keep', [0.9, 0.3])
def test_dropout_scale_is_float32_reciprocal(keep):
    s = P.dropout_scale(1000, keep, 1, 2)
    assert set(np.unique(s)) == {np.float32(0), np.float32(1) / np.float32(keep)}


@pytest.mark.parametrize('first', [0, 4, 1000, 4 * (1 << 32) - 8])
def test_dropout_scale_sub_range_is_the_whole_arrays_slice(first):
    whole = P.dropout_scale(first + 40, 0.6, 77, 1000003 * 5 + 1) if first < 10000 else None
    part = P.dropout_scale(40, 0.6, 77, 1000003 * 5 + 1, first_elem=first)
    if whole is not None:
        np.testing.assert_array_equal(part, whole[first:])
    # rows of an unaligned start still read the lanes of their own element index
    odd = P.dropout_scale(37, 0.6, 77, 1000003 * 5 + 1, first_elem=first + 3)
    np.testing.assert_array_equal(odd, part[3:])


@pytest.mark.parametrize('keep', [0.9, 0.5, 0.1])
def test_dropout_scale_kept_fraction(keep):
    """binomial: the kept fraction of 2^20 elements within 6 standard deviations"""
    n = 1 << 20
    s = P.dropout_scale(n, keep, (1 << 33) + 1, (1 << 32) + 5)
    kf = np.float32(keep)
    sd = np.sqrt(float(kf) * (1 - float(kf)) / n)
    assert abs((s > 0).mean() - float(kf)) < 6 * sd


def test_dropout_scale_different_streams_differ():
    a = P.dropout_scale(4096, 0.5, 1, 10)
    assert not np.array_equal(a, P.dropout_scale(4096, 0.5, 1, 11))
    assert not np.array_equal(a, P.dropout_scale(4096, 0.5, 2, 10))
    assert not np.array_equal(a, P.dropout_scale(4096, 0.5, 1, 10 + (1 << 32)))    # the high offset word counts


def test_gaussian_layout_and_values():
    """element 4 i + (0, 1, 2, 3) = (ra cos, ra sin, rb cos, rb sin) of group i's words"""
    seed, offset = 3 | (4 << 32), 9 | (2 << 32)
    z, rad = P.gaussian(11, seed, offset, with_radius=True)
    np.testing.assert_array_equal(P.gaussian(11, seed, offset), z)
    for i in range(3):
        r = P.philox4x32_10(np.array([i, 0, 9, 2], np.uint32), np.array([3, 4], np.uint32))
        u = P.u01(r)
        ra, rb = np.sqrt(-2 * np.log(1 - u[0])), np.sqrt(-2 * np.log(1 - u[2]))
        want = [ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]),
                rb * np.cos(2 * np.pi * u[3]), rb * np.sin(2 * np.pi * u[3])]
        for j in range(4):
            if 4 * i + j < 11:
                assert z[4 * i + j] == want[j]
                assert rad[4 * i + j] == (ra if j < 2 else rb)
    assert np.all(np.isfinite(z))


def test_gaussian_moments():
    """2^20 values: mean, variance, skewness and excess kurtosis within 6 standard errors of N(0, 1)"""
    n = 1 << 20
    z = P.gaussian(n, 17, (1 << 32) - 1)
    assert abs(z.mean()) < 6 / np.sqrt(n)
    assert abs(z.var() - 1) < 6 * np.sqrt(2.0 / n)
    assert abs(np.mean(z ** 3)) < 6 * np.sqrt(15.0 / n)
    assert abs(np.mean(z ** 4) - 3) < 6 * np.sqrt(96.0 / n)
    # the tails: |z| > 3 with probability 0.0027
    p = np.mean(np.abs(z) > 3)
    assert abs(p - 0.0026998) < 6 * np.sqrt(0.0027 / n)
