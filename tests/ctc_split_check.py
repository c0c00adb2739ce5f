"""Cases and child-process body of tests/test_hip_ctc_split.py: ctc_wave_split_kernel (the alpha and the beta sweep
side by side, csrc/ctc.hip) against ctc_wave_kernel (one wave runs both sweeps; NABU_CTC_WAVE_SERIAL=1, read once per
process, so the old kernel runs in a child process).

CASES: the table of tests/ctc_cases.py as far as the wave kernels take it, and on top of it
  grid   T in {1, 2, 3, 64, 65} x L in {0, 1, 31, 32, 63} x C in {2, 40, 64, 300}, three utterances each:
         0: logit_len = T, label_len = L, the first two labels equal (C = 2 has one label: all equal)
         1: logit_len = T - 1 (< T where T > 1), as many labels as fit
         2: logit_len = T, min(L, T) / 2 labels: a lattice with several alignments wherever T > 1.  judge() allows a
            multiple of the float32 oracle's own error on the batch, and that error is zero where every utterance has a
            single alignment (its sums cancel exactly); the table of tests/ctc_cases.py keeps a loose full-length
            utterance in every batch for this reason, and so does the grid
         where utterance 0 does not fit (T < L + repeats) the case is an INFEASIBLE one: utterance 0 must come back
         with nll = +inf, a zero gradient and its number in the status word, the others as valid as ever
  mixed  one batch whose utterances differ in all of these, and the same batch with one infeasible utterance
As a program: python tests/ctc_split_check.py OUT.npz — runs every case on the kernel this process dispatches to and
writes nll / dlogits / status per case."""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

from tests import ctc_cases as cc  # noqa: E402

SPLIT_WAVES = 16


def split_lds_bytes(T, C, Lmax):
    """ctc_split_lds_bytes of csrc/ctc.hip"""
    Smax = 2 * Lmax + 1
    return (T * C + 2 * T * Smax + SPLIT_WAVES * (64 + C) + 2) * 4 + 128 * 4


def split_eligible(T, C, Lmax):
    return Lmax <= 63 and split_lds_bytes(T, C, Lmax) <= 150 * 1024


def _labels(rng, C, L, repeat):
    lab = rng.integers(0, C - 1, L)
    if repeat and L >= 2:
        lab[1] = lab[0]
    return lab


def _fit(rng, C, L, Tb, repeat):
    """the longest prefix of a drawn label sequence that has an alignment over Tb frames"""
    lab = _labels(rng, C, L, repeat)
    while len(lab) and cc.needed_frames(lab[None, :], [len(lab)])[0] > Tb:
        lab = lab[:-1]
    return lab


def _case(logits, logit_len, labs, Lmax, meta):
    B = len(labs)
    labels = np.zeros((B, Lmax), np.int32)
    for b, lab in enumerate(labs):
        labels[b, :len(lab)] = lab
    label_len = np.array([len(lab) for lab in labs], np.int32)
    need = cc.needed_frames(labels, label_len)
    return cc.Case(np.ascontiguousarray(logits, np.float32), np.asarray(logit_len, np.int32), labels, label_len, need, meta)


def grid_case(T, L, C):
    rng = np.random.default_rng(1000003 * T + 1009 * L + C)
    logits = 2.0 * rng.standard_normal((3, T, C))
    lens = [T, max(1, T - 1), T]
    labs = [_labels(rng, C, L, True), _fit(rng, C, L, lens[1], False), _fit(rng, C, min(L // 2, T // 2), lens[2], True)]
    return _case(logits, lens, labs, L, dict(T=T, L=L, C=C))


def mixed_case(infeasible):
    rng = np.random.default_rng(77)
    T, C, Lmax = 65, 40, 63
    lens = [65, 1, 64, 3, 40, 2]
    labs = [_labels(rng, C, 32, True), _labels(rng, C, 0, False), _fit(rng, C, 63, 64, False),
            np.array([5, 5]), _fit(rng, C, 31, 40, True), _labels(rng, C, 1, False)]
    if infeasible:
        labs[3] = np.array([5, 5, 5])          # needs 5 frames, has 3
    return _case(2.0 * rng.standard_normal((len(lens), T, C)), lens, labs, Lmax, dict(mixed=True))


def _cases():
    out = []
    for e in cc.CASES:
        if cc.wave_eligible(*e['shape'][1:]):
            out.append(dict(id='table-' + e['id'], entry=e, scale=e['grad_scale']))
    for T in (1, 2, 3, 64, 65):
        for L in (0, 1, 31, 32, 63):
            for C in (2, 40, 64, 300):
                out.append(dict(id='grid-T%d-L%d-C%d' % (T, L, C), grid=(T, L, C), scale=1.0))
    out.append(dict(id='mixed', mixed=False, scale=0.37))
    out.append(dict(id='mixed-infeasible', mixed=True, scale=0.37))
    return out


CASES = _cases()
_built = {}


def build(c):
    """the Case of an entry of CASES (kept: the float64 oracle of a case is computed once)"""
    if c['id'] not in _built:
        _built[c['id']] = cc.build(c['entry']) if 'entry' in c else grid_case(*c['grid']) if 'grid' in c else mixed_case(c['mixed'])
    return _built[c['id']]


def infeasible(case):
    """the utterances without an alignment"""
    return np.flatnonzero(case.need > case.logit_len)


def main(argv):
    from tests import ctc_kernel_check as kc
    out = {}
    for c in CASES:
        case = build(c)
        nll, dl, status = kc.run(case.logits, case.logit_len, case.labels, case.label_len, c['scale'])
        out[c['id'] + '/nll'], out[c['id'] + '/dl'], out[c['id'] + '/status'] = nll, dl, np.int32(status)
    np.savez(argv[0], **out)
    print('CTC SPLIT CHILD OK %d cases' % len(CASES))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
