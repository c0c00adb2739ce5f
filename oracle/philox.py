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
