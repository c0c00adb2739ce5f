"""Records the bits of the parameter-update kernels (clip, accumulate, the Adam step and its norm-scaled form) on the device.

    python tests/golden/make_update_bits.py [out.npz]      # default: update_bits.npz next to this file; needs the GPU

PROVENANCE.  Unlike the other fixtures these numbers come from no oracle: they are what the library of the commit named in
LABNOTES.md ("One Adam kernel") wrote on an MI355X, and tests/test_hip_update_bits.py holds every later library to them
bit for bit.  The roundings of the Adam update are a choice (which products are fused), not a consequence of the formula,
and a float64 reference cannot tell two such choices apart; a recording can.  Re-record only when a change of the update's
bits is intended, from the library that makes it, and say so where the change is described.

Inputs are words of a splitmix64 sequence written out in uint64 arithmetic and cut into float32 fields, so they are the
same on every machine and with every numpy; the fixture keeps a digest of them per size.  cases(n) makes the calls and is
shared with the test.  For n <= FULL every output is kept whole, for the large size its SHA-256."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# 1..3: the scalar tail alone (threads 0..2 of block 0); 4, 5, 7, 8: one and two 16-byte groups with tails of 0, 1 and 3;
# 1030: two blocks and a tail of 2; 2 097 175 = 4 (2048 * 256 + 5) + 3: the grid-stride loop takes a second trip, then a tail
SIZES = [1, 2, 3, 4, 5, 7, 8, 1030, 2097175]
FULL = 1030
LR_T, ADAM = 2.5e-3, (0.9, 0.999, 1e-8)
SIXTH = float(np.float32(1.0) / np.float32(6.0))
GRAD_SCALES = (('sixth', SIXTH), ('one', 1.0))
CLIPS = (('1', 1.0), ('inf', float('inf')))
NAN_BITS = 0x7FC00000
GARBAGE = -123.0                                                     # what param_out holds before a step that reads src


def words(n, stream):
    """n uint32 words: the high halves of splitmix64 at the states (stream << 32) + (i + 1) * 0x9E3779B97F4A7C15"""
    z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + (np.uint64(stream) << np.uint64(32))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def fields(w, lo, hi, signed):
    """float32 bit patterns: biased exponent lo + (bits 23..30 of w) % (hi - lo + 1), the fraction and, if signed, the
    sign of w"""
    e = np.uint32(lo) + ((w >> np.uint32(23)) & np.uint32(0xFF)) % np.uint32(hi - lo + 1)
    b = (e << np.uint32(23)) | (w & np.uint32(0x7FFFFF))
    return b | (w & np.uint32(0x80000000)) if signed else b


def inputs(n):
    """{name: uint32[n]} of p, g, acc, m, v, another draw for each n.
    g, acc: |x| in [2^-8, 2^4), so |g * grad_scale| lies on both sides of clip = 1 at both scales; where i % 16 is 8..10 both
    are tiny (2^-77 .. 2^-46) so that the special v next to them stays tiny.  g holds a NaN, a +inf and a -0.0 in every 64.
    m: both signs, 2^-12 .. 2^2.  p: both signs, 2^-7 .. 2^2.
    v >= 0: i % 8 == 0 exactly 0, 1 denormal, 2 in [2^-126, 2^-96) (below sqrtf's rescaling threshold), else 2^-20 .. 2^3."""
    i = np.arange(n)
    w = {k: words(n, 8 * n + s) for s, k in enumerate(('p', 'g', 'acc', 'm', 'v'))}
    tiny = (i % 16 >= 8) & (i % 16 < 11)
    x = {k: np.where(tiny, fields(w[k], 50, 80, True), fields(w[k], 119, 130, True)) for k in ('g', 'acc')}
    for at, pattern in ((5, NAN_BITS), (6, 0x7F800000), (7, 0x80000000)):
        x['g'][i % 64 == at] = pattern
    x['m'] = fields(w['m'], 115, 128, True)
    x['p'] = fields(w['p'], 120, 128, True)
    v = fields(w['v'], 107, 129, False)
    v[i % 8 == 0] = 0
    v = np.where(i % 8 == 1, (w['v'] & np.uint32(0x7FFFFF)) | np.uint32(1), v)
    x['v'] = np.where(i % 8 == 2, fields(w['v'], 1, 30, False), v)
    return {k: np.ascontiguousarray(a, dtype=np.uint32) for k, a in x.items()}


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def cases(n):
    """yields ('<ops.py entry point>:<arguments>', {array name: device tensor written by the call}), every call on fresh
    copies of the inputs of inputs(n)"""
    import torch
    from nabu_amd import ops as hip
    d = {k: torch.from_numpy(a.view(np.float32)).cuda() for k, a in inputs(n).items()}
    g, acc = d['g'], d['acc']

    def state(from_src):
        return [torch.full_like(d['p'], GARBAGE) if from_src else d['p'].clone(), d['m'].clone(), d['v'].clone()]

    def written(s):
        return dict(zip(('p', 'm', 'v'), s))
    for sname, gs in GRAD_SCALES:
        for cname, clip in CLIPS:
            tag = ':scale_%s_clip_%s' % (sname, cname)
            s = state(False)
            hip.adam_clip_step(s[0], g, s[1], s[2], LR_T, *ADAM, clip, gs)
            yield 'adam_clip_step' + tag, written(s)
            s = state(True)
            hip.adam_clip_step_from(s[0], d['p'], g, s[1], s[2], LR_T, *ADAM, clip, gs)
            yield 'adam_clip_step_from' + tag, written(s)
            for from_src in (False, True):
                s = state(from_src)
                hip.adam_clip_step_acc(s[0], d['p'] if from_src else None, acc, g, s[1], s[2], LR_T, *ADAM, clip, gs)
                yield 'adam_clip_step_acc' + tag + ('_src' if from_src else ''), written(s)
    for fname, factor in (('sixth', int(np.float32(SIXTH).view(np.uint32))), ('nan', NAN_BITS)):
        stats = torch.tensor([0, factor, 0, 0], dtype=torch.int32).cuda()
        for from_src in (False, True):
            for with_acc in (False, True):
                s = state(from_src)
                hip.adam_scaled_step(s[0], d['p'] if from_src else None, acc if with_acc else None, g, s[1], s[2], LR_T,
                                     *ADAM, stats)
                yield ('adam_scaled_step:factor_%s%s%s' % (fname, '_src' if from_src else '', '_acc' if with_acc else ''),
                       written(s))
    for cname, clip in CLIPS:
        tag = ':clip_' + cname
        yield 'clip_' + tag, {'g': hip.clip_(g.clone(), clip)}
        out = g.clone()
        yield 'clip_accumulate' + tag + '_out_is_g', {'out': hip.clip_accumulate(out, None, out, clip)}
        out = acc.clone()
        yield 'clip_accumulate' + tag + '_out_is_acc', {'out': hip.clip_accumulate(out, out, g, clip)}
        yield 'clip_accumulate' + tag + '_separate', {'out': hip.clip_accumulate(torch.full_like(g, GARBAGE), acc, g, clip)}


def record():
    out = {}
    for n in SIZES:
        x = inputs(n)
        out['%d|inputs' % n] = digest(x[k] for k in sorted(x))
        for name, arrays in cases(n):
            for k, t in arrays.items():
                out['%d|%s|%s' % (n, name, k)] = bits(t) if n <= FULL else digest([bits(t)])
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'update_bits.npz')
    fixture = record()
    np.savez_compressed(path, **fixture)
    print('%d arrays, %d bytes -> %s' % (len(fixture), os.path.getsize(path), path))
