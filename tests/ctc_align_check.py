"""Cases of tests/test_hip_ctc_align.py and what is checked on them; importable without a GPU.

As a program (a child process started with NABU_CTC_ALIGN_WORKGROUP=1, which csrc/ctc_align.hip reads once per
process) it runs every wave-eligible grid case on the workgroup route and saves the five outputs of each to an .npz:
the parent compares them with the bits its own, default-route run produced.
usage: python tests/ctc_align_check.py OUT.npz"""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

from tests import ctc_align_ref as ar  # noqa: E402
from tests import ctc_cases as cc  # noqa: E402

# (B, T, C, Lmax) of the issue, then two shapes whose back-pointers no longer fit the LDS and go to the workspace:
# workgroup route 700 * 261 B = 178 KiB, wave route (3 * 4000 + 128) * 4 + 250 * 512 B = 172 KiB
GRID_SHAPES = [(4, 12, 5, 3), (3, 40, 65, 10), (2, 150, 41, 63), (2, 150, 41, 64), (2, 300, 41, 130),
               (2, 1000, 40, 50), (2, 700, 5, 130), (2, 4000, 3, 2)]
GRID = [(s, lat) for s in GRID_SHAPES for lat in cc.LATTICES]
CONTINUOUS = [(s, r) for s in [(4, 40, 65, 10), (2, 150, 41, 63), (2, 150, 41, 64)] for r in cc.REGIMES]
LDS_MAX = 150 * 1024


def grid_id(entry):
    return '%dx%dx%dx%d-%s' % (entry[0] + (entry[1],))


def wave_eligible(T, Lmax):
    """the dispatch of nabu_ctc_align without the switch: one wave64 per utterance"""
    return Lmax <= 63 and (3 * T + T % 2 + 128) * 4 <= LDS_MAX


def backpointers_in_lds(T, Lmax, wave):
    if wave:
        return (3 * T + T % 2 + 128) * 4 + (T + 15) // 16 * 512 <= LDS_MAX
    return (2 * T + 2 * max(Lmax, 1) + 3 * (2 * Lmax + 1)) * 4 + T * (2 * Lmax + 1) <= LDS_MAX


def forced_workgroup():
    return os.environ.get('NABU_CTC_ALIGN_WORKGROUP', '0') not in ('', '0')


def grid_case(shape, lattice):
    """lengths and labels of ctc_cases.make_case (utterance 0: full length and an adjacent repeat, the last:
    label_len = Lmax, utterance 1: L = 0 when B >= 3; 'tight': logit_len = L + repeats for all but utterance 0), the
    logits drawn on the quarter grid; at least one utterance shorter than T; B = 4 also gets the planted rows"""
    B, T, C, Lmax = shape
    c = cc.make_case(B, T, C, Lmax, 'random', lattice, cc.seed_of(*shape))
    rng = np.random.default_rng([cc.seed_of(*shape), 7])
    logits = ar.grid_logits(rng, (B, T, C))
    logit_len, labels, label_len = c.logit_len.copy(), c.labels.copy(), c.label_len.copy()
    if np.all(logit_len == T):
        logit_len[-1] = max(int(c.need[-1]), T - 3)
    if B == 4:
        assert label_len[1] == 0                                      # L = 0
        label_len[2], logit_len[2] = 1, 1                             # L = 1 with Tb = 1
        labels[3, :3], label_len[3], logit_len[3] = labels[3, 0], 3, 5     # one label three times, Tb = 5: one path
    assert np.any(logit_len < T)
    return logits, logit_len.astype(np.int32), labels.astype(np.int32), label_len.astype(np.int32)


def continuous_case(shape, regime):
    B, T, C, Lmax = shape
    c = cc.make_case(B, T, C, Lmax, regime, 'loose', cc.seed_of(*shape))
    return c.logits, c.logit_len, c.labels, c.label_len


def run(logits, logit_len, labels, label_len):
    """one call of ops.ctc_align on host arrays -> the five outputs as NumPy arrays (status an int)"""
    import torch
    from nabu_amd import ops

    def dev(a, dtype):
        return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()
    state, seg, conf, score, status = ops.ctc_align(dev(logits, torch.float32), dev(logit_len, torch.int32),
                                                    dev(labels, torch.int32), dev(label_len, torch.int32))
    return state.cpu().numpy(), seg.cpu().numpy(), conf.cpu().numpy(), score.cpu().numpy(), int(status.item())


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.int32) if np.asarray(x).dtype == np.float32 else np.asarray(x),
                              np.asarray(y).view(np.int32) if np.asarray(y).dtype == np.float32 else np.asarray(y))
               for x, y in zip(a, b))


def _rel(err, ref):
    return float(np.max(np.where(ref != 0, err / np.where(ref != 0, np.abs(ref), 1.0), err))) if err.size else 0.0


def scalar_failures(case, out, k=cc.K_NLL, judge_floor=False):
    """score and conf of a result against the float64 values of ITS OWN path.  The statistic is judge()'s for the nll:
    the largest relative error of the case; the allowance is k = ctc_cases.K_NLL times the same statistic of the
    float32 twin (its score and conf against the float64 values of the twin's own path).  Where the twin's error is
    exactly 0 the floor 4 * U * sum|terms| / |value| stands in its place (4 roundings of the size of the summed terms).
    judge_floor (the grid and rejected-input cases, whose yardstick is the exact path; their scalars are an extra
    check): ctc_cases.judge()'s form for the nll, k * twin + 4 * U — a float32 result is 0.5 ulp from the truth in the
    worst case whatever the arithmetic, while one draw of the twin may land on it by chance (seen: (2, 4000, 3, 2)
    tight, twin 0.05 ulp, kernel 1.02 ulp).
    Returns (failures, figures)."""
    logits, logit_len, labels, label_len = case
    state, seg, conf, score, _ = out
    s64, c64, _, sabs, _ = ar.path_values(logits, logit_len, labels, label_len, state)
    st32, _, c32, s32, _ = ar.align(logits, logit_len, labels, label_len, np.float32)
    t64, tc64, _, _, _ = ar.path_values(logits, logit_len, labels, label_len, st32)
    ok = np.isfinite(s32.astype(np.float64))
    live = np.asarray(seg)[..., 0] >= 0
    e_ref_s = _rel(np.abs(s32.astype(np.float64) - t64)[ok], t64[ok])
    e_ker_s = _rel(np.abs(score.astype(np.float64) - s64)[ok], s64[ok])
    e_ref_c = _rel(np.abs(c32.astype(np.float64) - tc64)[live], tc64[live])
    e_ker_c = _rel(np.abs(conf.astype(np.float64) - c64)[live], c64[live])
    floor = 4 * cc.U * _rel(sabs[ok], s64[ok])
    if judge_floor:
        tol_s, tol_c = k * e_ref_s + 4 * cc.U, k * e_ref_c + 4 * cc.U
    else:
        tol_s = k * e_ref_s if e_ref_s > 0 else floor
        tol_c = k * e_ref_c if e_ref_c > 0 else floor
    bad = []
    if not e_ker_s <= tol_s:
        bad.append('score: %.3e > %.3e (twin %.3e)' % (e_ker_s, tol_s, e_ref_s))
    if not e_ker_c <= tol_c:
        bad.append('conf: %.3e > %.3e (twin %.3e)' % (e_ker_c, tol_c, e_ref_c))
    return bad, 'score %.3e / twin %.3e, conf %.3e / twin %.3e' % (e_ker_s, e_ref_s, e_ker_c, e_ref_c)


def main(argv):
    assert forced_workgroup(), 'run with NABU_CTC_ALIGN_WORKGROUP=1'
    saved = {}
    for entry in GRID:
        (B, T, C, Lmax), _ = entry
        if not wave_eligible(T, Lmax):
            continue
        out = run(*grid_case(*entry))
        for name, a in zip(('state', 'seg', 'conf', 'score', 'status'), out):
            saved['%s/%s' % (grid_id(entry), name)] = np.asarray(a)
        print('CASE %s workgroup status %d' % (grid_id(entry), out[4]), flush=True)
    np.savez(argv[0], **saved)
    print('ALIGN DONE %d arrays' % len(saved))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
