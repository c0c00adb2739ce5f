"""Host reference of the project's counter-based random stream (Philox4x32-10,
csrc/common.h) and of the scheduled-sampling draw built on it.

Everything is exact 32-bit integer arithmetic in NumPy, vectorised over the
counters, so the host reproduces the device's words bit for bit.  The sampling
draw itself (reference_draw) takes its inverse CDF in float64: where the device's
float32 sums may legitimately land on the other side of a class boundary, the
returned distance to the nearest boundary lets a test tell such rows apart."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other), uint32 -> [..., 4] uint32.

    Ten rounds of (x, y, z, w) -> (hi(M1 z) ^ y ^ k0, lo(M1 z), hi(M0 x) ^ w ^ k1, lo(M0 x)),
    the key bumped by the Weyl constants after every round (the bump after the tenth is unused)."""
    ctr = np.asarray(ctr, np.uint32)
    key = np.asarray(key, np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    x, y, z, w = (np.broadcast_to(ctr[..., i], shape).astype(np.uint32) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape).astype(np.uint32) for i in range(2))
    with np.errstate(over='ignore'):
        for _ in range(10):
            p0 = M0 * x.astype(np.uint64)
            p1 = M1 * z.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _LO).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _LO).astype(np.uint32)
            x, y, z, w = hi1 ^ y ^ k0, lo1, hi0 ^ w ^ k1, lo0
            k0 = k0 + W0
            k1 = k1 + W1
    return np.stack([x, y, z, w], -1)


def u01(x):
    """(x >> 8) * 2^-24: the float32 uniform in [0, 1) of one word (exact in float32 and float64)"""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def sample_words(rows, seed, offset):
    """words (x, y) of the scheduled-sampling draw of each global row: counter (row, 0, offset_lo, offset_hi),
    key (seed_lo, seed_hi); x decides the Bernoulli, y is the uniform of the inverse CDF"""
    rows = np.asarray(rows, np.int64)
    ctr = np.zeros(rows.shape + (4,), np.uint32)
    ctr[..., 0] = (rows & 0xFFFFFFFF).astype(np.uint32)
    ctr[..., 2] = np.uint32(offset & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32((offset >> 32) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    r = philox4x32_10(ctr, key)
    return r[..., 0], r[..., 1]


def reference_draw(logits, prob, seed, offset, teacher, row0=0):
    """The ids scheduled sampling should produce for logits [B, C] at (seed, offset), rows row0 .. row0 + B - 1.

    Returns (ids [B] int64, selected [B] bool, margin [B] float64, bounds [B, 2] int64):
      selected: u01(x) < prob, compared exactly as the device compares float32 values;
      ids: the teacher id where not selected, else the first class c whose float64 cumulative softmax sum
           exceeds u01(y) * total (C - 1 if none does);
      margin: |u01(y) * total - nearest cumulative sum| / total (inf for rows not selected);
      bounds: for selected rows the first and last class whose CDF interval reaches within 1e-5 * total of
              u01(y) * total -- the classes a float32 evaluation of the same draw may land on."""
    lg = np.asarray(logits, np.float64)
    B, C = lg.shape
    x, y = sample_words(np.arange(B, dtype=np.int64) + row0, seed, offset)
    selected = u01(x) < np.float64(np.float32(prob))
    e = np.exp(lg - lg.max(1, keepdims=True))
    cum = np.cumsum(e, 1)
    total = cum[:, -1]
    target = u01(y) * total
    drawn = np.minimum((cum > target[:, None]).argmax(1), C - 1)
    drawn = np.where((cum > target[:, None]).any(1), drawn, C - 1)
    margin = np.abs(cum - target[:, None]).min(1) / total
    tol = 1e-5 * total
    lo = np.minimum(((cum > (target - tol)[:, None])).argmax(1), C - 1)
    hi_hit = cum > (target + tol)[:, None]
    hi = np.where(hi_hit.any(1), hi_hit.argmax(1), C - 1)
    ids = np.where(selected, drawn, np.asarray(teacher, np.int64))
    margin = np.where(selected, margin, np.inf)
    return ids, selected, margin, np.stack([lo, hi], 1)


def _group_words(groups, seed, offset):
    """words [len(groups), 4] of the element-wise stream: counter (group_lo, group_hi, offset_lo, offset_hi),
    key (seed_lo, seed_hi) -- dropout_kernel / gaussian_noise_kernel of elementwise.hip, dropout_scale4 of common.h"""
    groups = np.asarray(groups, np.uint64)
    ctr = np.zeros(groups.shape + (4,), np.uint32)
    ctr[..., 0] = (groups & _LO).astype(np.uint32)
    ctr[..., 1] = (groups >> np.uint64(32)).astype(np.uint32)
    ctr[..., 2] = np.uint32(offset & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32((offset >> 32) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    return philox4x32_10(ctr, key)


def dropout_scale(n, keep, seed, offset, first_elem=0):
    """float32 [n]: the dropout scale factors (0 or float32(1) / float32(keep)) of elements first_elem ..
    first_elem + n - 1 of the array the stream (seed, offset) is defined on.  Element e reads lane e % 4 of the
    words of group e // 4 and is kept when u01(word) < float32(keep), as the device compares float32 values."""
    e = np.arange(first_elem, first_elem + n, dtype=np.uint64)
    if n == 0:
        return np.zeros(0, np.float32)
    g0 = int(e[0]) // 4
    words = _group_words(np.arange(g0, int(e[-1]) // 4 + 1, dtype=np.uint64), seed, offset).reshape(-1)
    w = words[(e - np.uint64(4 * g0)).astype(np.int64)]
    k = np.float32(keep)
    inv = np.float32(1) / k
    return np.where(u01(w) < np.float64(k), inv, np.float32(0)).astype(np.float32)


def gaussian(n, seed, offset, with_radius=False):
    """float64 [n]: the standard normal values gaussian_noise_kernel adds (times stddev) to elements 0 .. n - 1.
    Group i's words (x, y, z, w) give Box-Muller pairs on u1 = 1 - u01(x), u2 = u01(y) and u3 = 1 - u01(z),
    u4 = u01(w), in the order (ra cos 2 pi u2, ra sin 2 pi u2, rb cos 2 pi u4, rb sin 2 pi u4), ra = sqrt(-2 ln u1),
    rb = sqrt(-2 ln u3) -- in float64 from the device's exact uniforms.  with_radius: also return each element's
    radius (ra or rb), the factor by which an error in the float32 angle 2 pi u reaches the value."""
    if n == 0:
        return (np.zeros(0), np.zeros(0)) if with_radius else np.zeros(0)
    r = _group_words(np.arange((n + 3) // 4, dtype=np.uint64), seed, offset)
    u1, u2, u3, u4 = 1.0 - u01(r[:, 0]), u01(r[:, 1]), 1.0 - u01(r[:, 2]), u01(r[:, 3])
    ra, rb = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    a, b = 2.0 * np.pi * u2, 2.0 * np.pi * u4
    z = np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], 1).reshape(-1)[:n]
    rad = np.stack([ra, ra, rb, rb], 1).reshape(-1)[:n]
    return (z, rad) if with_radius else z
