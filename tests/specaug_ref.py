"""Host reference of SpecAugment on the device (nabu_spec_augment_f32; the rules: DESIGN.md, "SpecAugment") in NumPy on the
host Philox of oracle/philox.py.  Every choice is integer arithmetic, so the parameters equal the device's exactly; so
does the result of the masks.  The warp's interpolation is returned in float64 from the float32 weight the device uses.

A policy is anything with the fields of nabu_amd.ops.SpecAugmentPolicy (Policy below is one without the package)."""
import collections

import numpy as np

from oracle import philox as P

Policy = collections.namedtuple('Policy', ['time_warp', 'time_masks', 'time_mask_width', 'time_mask_ratio', 'freq_masks',
                                           'freq_mask_width', 'feature_blocks'])
OFF = Policy(0, 0, 0, 1.0, 0, 0, 1)


def words(b, k, seed, offset):
    """the four words of utterance b's draw k: counter (b, k, offset_lo, offset_hi), key (seed_lo, seed_hi)"""
    ctr = np.array([b, k, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF], np.uint32)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    return [int(v) for v in P.philox4x32_10(ctr, key)]


def below(w, m):
    """uniform integer in [0, m) from one 32-bit word (Python integers: exact)"""
    return ((int(w) >> 8) * int(m)) >> 24


def param_width(policy):
    return 2 + 2 * policy.time_masks + 2 * policy.freq_masks


def draw(b, n, D, policy, seed, offset):
    """utterance b of n frames: (c, c') ((0, 0): not warped), [(t0, t)] time masks, [(f0, f)] frequency masks"""
    W, dblk = policy.time_warp, D // policy.feature_blocks
    c = cp = 0
    if W > 0 and n >= 2 * W + 3:
        w = words(b, 0, seed, offset)
        c = W + 1 + below(w[0], n - 2 * W - 2)
        cp = c - W + below(w[1], 2 * W + 1)
    cap = min(policy.time_mask_width, int(np.float32(policy.time_mask_ratio) * np.float32(n)))
    tm, fm = [], []
    for j in range(policy.time_masks):
        w = words(b, 1 + j, seed, offset)
        t = below(w[0], cap + 1)
        tm.append((below(w[1], n - t + 1), t))
    for j in range(policy.freq_masks):
        w = words(b, 1 + policy.time_masks + j, seed, offset)
        f = below(w[0], min(policy.freq_mask_width, dblk) + 1)
        fm.append((below(w[1], dblk - f + 1), f))
    return (c, cp), tm, fm


def params(lens, D, policy, seed, offset):
    """int32 [B, param_width]: what the device writes into its parameter buffer"""
    out = np.zeros((len(lens), param_width(policy)), np.int32)
    for b, n in enumerate(lens):
        (c, cp), tm, fm = draw(b, int(n), D, policy, seed, offset)
        out[b] = [c, cp] + [v for m in tm for v in m] + [v for m in fm for v in m]
    return out


def warp_source(t, n, c, cp):
    """output frame t of a warped utterance reads source position i + r / den: (i, r, den), Python integers"""
    if t < cp:
        num, den = t * c, cp
    else:
        num, den = c * (n - 1 - cp) + (t - cp) * (n - 1 - c), n - 1 - cp
    return num // den, num % den, den


def augment(x, lens, policy, seed, offset):
    """x [B, T, D] float32 -> (y float64 [B, T, D], params, frac float32 [B, T], span float64 [B, T, D]):
    y = a + frac (b - a) in float64 from the float32 frames a = x[i], b = x[i + 1] and the float32 weight frac = r / den
    (y = a where r = 0: exact), zero inside the masks, x in the frames t >= len; span = frac |b - a| outside the masks
    (what the rounding of b - a is scaled by)"""
    x = np.asarray(x, np.float32)
    B, T, D = x.shape
    dblk = D // policy.feature_blocks
    y = x.astype(np.float64)
    frac = np.zeros((B, T), np.float32)
    span = np.zeros((B, T, D))
    prm = params(lens, D, policy, seed, offset)
    for b in range(B):
        n = int(lens[b])
        (c, cp), tm, fm = draw(b, n, D, policy, seed, offset)
        if c:
            for t in range(n):
                i, r, den = warp_source(t, n, c, cp)
                if r:
                    frac[b, t] = np.float32(r) / np.float32(den)
                    a, nxt = x[b, i].astype(np.float64), x[b, i + 1].astype(np.float64)
                    y[b, t] = a + np.float64(frac[b, t]) * (nxt - a)
                    span[b, t] = np.float64(frac[b, t]) * np.abs(nxt - a)
                else:
                    y[b, t] = x[b, i]
        for t0, t in tm:
            y[b, t0:t0 + t] = 0
            span[b, t0:t0 + t] = 0
        cols = np.zeros(dblk, bool)
        for f0, f in fm:
            cols[f0:f0 + f] = True
        cols = np.tile(cols, policy.feature_blocks)
        y[b, :n, cols] = 0
        span[b, :n, cols] = 0
    return y, prm, frac, span
