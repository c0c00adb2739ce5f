"""Cases of tests/test_hip_transducer_align.py and what is checked on them; importable without a GPU.

As a program (a child process started with NABU_TRANSDUCER_ALIGN_WORKGROUP=1, which csrc/transducer_align.hip reads
once per process) it runs every wave-eligible grid case on the workgroup route and saves the five outputs of each to
an .npz: the parent compares them with the bits its own, default-route run produced.
usage: python tests/transducer_align_check.py OUT.npz"""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

from tests import transducer_align_ref as ar  # noqa: E402
from tests import transducer_cases as tc  # noqa: E402

# the shapes (B, T, C, Lmax) of the loss's tests; the grid needs a spare class, so C >= 3
GRID_SHAPES = [s for s in tc.ALL_SHAPES if s[2] >= 3]
CONTINUOUS = [(s, r) for s in [(4, 70, 40, 63), (4, 70, 40, 64), (3, 12, 65, 6)] for r in tc.REGIMES]
LDS_MAX = 150 * 1024
NAMES = ('state', 'frame', 'conf', 'score', 'status')


def shape_id(shape):
    return '%dx%dx%dx%d' % tuple(shape)


def wave_eligible(Lmax):
    """the dispatch of nabu_transducer_align without the switch: one wave64 per utterance"""
    return Lmax + 1 <= 64


def forced_workgroup():
    return os.environ.get('NABU_TRANSDUCER_ALIGN_WORKGROUP', '0') not in ('', '0')


class GridCase(object):
    def __init__(self, inputs, ref64, ref32):
        self.inputs, self.ref64, self.ref32 = inputs, ref64, ref32


_grid = {}


def grid_draw(shape):
    """(inputs, float64 restatement) of a shape's grid case.  A draw that meets no tie at a node with both
    predecessors pins nothing: the next seed is drawn until one does (shapes with one frame or without labels have no
    such node and take the first draw)."""
    for k in range(64):
        inputs = ar.grid_case(shape, tc.seed_of(*shape) + 1000003 * k)
        ref64 = ar.align(*inputs, dtype=np.float64)
        if ref64[5].sum() >= 1 or shape[1] < 2 or shape[3] < 1:
            return inputs, ref64
    raise AssertionError('no draw with a tie for %s' % (shape,))


def grid_reference(shape):
    """the grid case of a shape with its float64 and float32 restatements (computed once, shared, read-only)"""
    shape = tuple(shape)
    if shape not in _grid:
        inputs, ref64 = grid_draw(shape)
        ref32 = ar.align(*inputs, dtype=np.float32)
        for a in inputs + tuple(ref64[:4]) + tuple(ref32[:4]):
            a.setflags(write=False)
        _grid[shape] = GridCase(inputs, ref64, ref32)
    return _grid[shape]


def run(f, g, enc_len, labels, label_len):
    """one call of ops.transducer_align on host arrays -> the five outputs as NumPy arrays (status an int)"""
    import torch
    from nabu_amd import ops

    def dev(a, dtype):
        return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()
    out = ops.transducer_align(dev(f, torch.float32), dev(g, torch.float32), dev(enc_len, torch.int32),
                               dev(labels, torch.int32) if labels is not None else None, dev(label_len, torch.int32))
    return tuple(a.cpu().numpy() for a in out[:4]) + (int(out[4].item()),)


def same_bits(a, b):
    def raw(x):
        x = np.asarray(x)
        return x.view(np.int32) if x.dtype == np.float32 else x
    return all(np.array_equal(raw(x), raw(y)) for x, y in zip(a, b))


def _rel(err, ref):
    return float(np.max(np.where(ref != 0, err / np.where(ref != 0, np.abs(ref), 1.0), err))) if err.size else 0.0


def scalar_allowances(case, out, k=tc.K_NLL):
    """score and conf of a result against the float64 values of ITS OWN path — the yardstick of
    ctc_align_check.scalar_failures: the statistic is the largest relative error of the case, the allowance k =
    ctc_cases.K_NLL times the same statistic of the float32 restatement (its score and conf against the float64 values
    of its own path); where that is exactly 0, the floor 4 U sum|terms| / |value| stands in its place.
    Returns (failures, figures, absolute allowance of every utterance's score)."""
    f, g, enc_len, labels, label_len = case
    state, frame, conf, score, _ = out
    s64, c64, sabs = ar.path_values(f, g, enc_len, labels, label_len, frame)
    _, fr32, c32, s32, _, _ = ar.align(f, g, enc_len, labels, label_len, np.float32)
    t64, tc64, _ = ar.path_values(f, g, enc_len, labels, label_len, fr32)
    ok = np.isfinite(s32.astype(np.float64))
    live = np.asarray(frame) >= 0
    e_ref_s = _rel(np.abs(s32.astype(np.float64) - t64)[ok], t64[ok])
    e_ker_s = _rel(np.abs(score.astype(np.float64) - s64)[ok], s64[ok])
    e_ref_c = _rel(np.abs(c32.astype(np.float64) - tc64)[live], tc64[live])
    e_ker_c = _rel(np.abs(conf.astype(np.float64) - c64)[live], c64[live])
    floor = 4 * tc.U * _rel(sabs[ok], s64[ok])
    tol_s = k * e_ref_s if e_ref_s > 0 else floor
    tol_c = k * e_ref_c if e_ref_c > 0 else floor
    bad = []
    if not e_ker_s <= tol_s:
        bad.append('score: %.3e > %.3e (restatement %.3e)' % (e_ker_s, tol_s, e_ref_s))
    if not e_ker_c <= tol_c:
        bad.append('conf: %.3e > %.3e (restatement %.3e)' % (e_ker_c, tol_c, e_ref_c))
    figures = 'score %.3e / restatement %.3e, conf %.3e / restatement %.3e' % (e_ker_s, e_ref_s, e_ker_c, e_ref_c)
    return bad, figures, tol_s * np.abs(s64)


def main(argv):
    assert forced_workgroup(), 'run with NABU_TRANSDUCER_ALIGN_WORKGROUP=1'
    saved = {}
    for shape in GRID_SHAPES:
        if not wave_eligible(shape[3]):
            continue
        out = run(*grid_reference(shape).inputs)
        for name, a in zip(NAMES, out):
            saved['%s/%s' % (shape_id(shape), name)] = np.asarray(a)
        print('CASE %s workgroup status %d' % (shape_id(shape), out[4]), flush=True)
    np.savez(argv[0], **saved)
    print('ALIGN DONE %d arrays' % len(saved))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
