"""CPU tests of the forced-alignment yardstick (tests/ctc_align_ref.py) and of nabu_ctc_align's host-side contract.

The float64 restatement is held to brute force over every label string of tiny problems; the quarter grid the GPU
tests use for their exact comparison is shown to give the same path in float32 and float64; and the size query and
the three kinds of refusal of the entry point are exercised through the library without a device."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import ctc_align_check as ck
from tests import ctc_align_ref as ar


def _targets(C, maxL):
    for L in range(maxL + 1):
        for lab in itertools.product(range(C - 1), repeat=L):
            yield list(lab)


@pytest.mark.parametrize('T', [1, 2, 3, 4, 5, 6])
def test_float64_viterbi_equals_brute_force(T):
    """all C^T strings for C = 3, L <= 2 (repeated labels included), continuous and grid logits: the best score of the
    strings that collapse to the target is the restatement's, and the restatement's path collapses to the target"""
    C = 3
    rng = np.random.default_rng(100 + T)
    for draw in range(3):
        x = rng.standard_normal((T, C)) * 2 if draw < 2 else ar.grid_logits(rng, (T, C)).astype(np.float64)
        for lab in _targets(C, 2):
            best = ar.brute_force(x, lab)
            if not ar.valid(lab, T, C):
                assert best is None, (T, lab)
                continue
            path, v = ar.viterbi(x, lab)
            cls = ar.extended(lab, C - 1)[path]
            assert ar.collapse(cls, C - 1) == lab, (T, lab, path)
            assert not ar.check_path(path, T, lab, T), (T, lab, path)
            assert best is not None and abs(v - best) <= 1e-12 * max(1.0, abs(best)), (T, lab, v, best)
            assert abs(np.sum(x[np.arange(T), cls]) - best) <= 1e-12 * max(1.0, abs(best))


def test_tie_rule_on_constructed_frames():
    """all-equal logits: every reachable move ties.  The end is S-1 (S-2 would have to be strictly better); walking
    back, a state stays while its own value was reachable a frame earlier, then steps, and skips only where neither
    was: the path runs ahead as fast as the lattice allows and waits in the last blank"""
    x = np.zeros((6, 4))
    path, _ = ar.viterbi(x, [0, 1])
    assert path.tolist() == [1, 3, 4, 4, 4, 4]
    path, _ = ar.viterbi(x, [0, 0])          # no skip between equal labels
    assert path.tolist() == [1, 2, 3, 4, 4, 4]
    x[1, 0] = 1.0                            # staying in label 0 for a frame now pays: the skip comes a frame later
    path, _ = ar.viterbi(x, [0, 1])
    assert path.tolist() == [1, 1, 3, 4, 4, 4]
    path, _ = ar.viterbi(np.zeros((2, 4)), [0, 1])      # only the skip fits: 1 -> 3
    assert path.tolist() == [1, 3]
    path, _ = ar.viterbi(np.zeros((3, 4)), [])
    assert path.tolist() == [0, 0, 0]


@pytest.mark.parametrize('entry', ck.GRID, ids=[ck.grid_id(e) for e in ck.GRID])
def test_grid_logits_give_one_path_in_float32_and_float64(entry):
    """what makes the grid a fair exact test: checked, not assumed"""
    logits, logit_len, labels, label_len = ck.grid_case(*entry)
    (B, T, C, Lmax), _ = entry
    assert np.all(logits * 4 == np.round(logits * 4)) and np.abs(logits).max() <= 8
    for b in range(B):
        Tb, L = int(logit_len[b]), int(label_len[b])
        p64, v64 = ar.viterbi(logits[b, :Tb], labels[b, :L], np.float64)
        p32, v32 = ar.viterbi(logits[b, :Tb], labels[b, :L], np.float32)
        assert v32.dtype == np.float32 and float(v32) == float(v64), (b, v32, v64)
        assert np.array_equal(p32, p64), b


def test_grid_cases_hold_the_planted_rows():
    logits, logit_len, labels, label_len = ck.grid_case((4, 12, 5, 3), 'loose')
    assert label_len[1] == 0 and (label_len[2], logit_len[2]) == (1, 1)
    assert (label_len[3], logit_len[3]) == (3, 5) and len(set(labels[3, :3])) == 1
    state, seg, conf, score, status = ar.align(logits, logit_len, labels, label_len)
    assert status == 0 and np.all(state[1, :logit_len[1]] == 0) and state[2, 0] == 1
    assert state[3, :5].tolist() == [1, 2, 3, 4, 5] and np.all(state[3, 5:] == -1)
    assert seg[3].tolist() == [[0, 1], [2, 3], [4, 5]]
    for shape, lat in ck.GRID:
        if lat == 'tight':
            _, tl, lab, ll = ck.grid_case(shape, lat)
            for b in range(1, shape[0]):
                if shape[0] == 4 and b >= 2:
                    continue
                row = lab[b, :ll[b]]
                assert tl[b] == max(1, len(row) + int(np.sum(row[1:] == row[:-1])))
    # the two shapes added for the workspace back-pointers do leave the LDS, the issue's shapes stay inside
    for (B, T, C, Lmax) in ck.GRID_SHAPES:
        wave = ck.wave_eligible(T, Lmax)
        assert ck.backpointers_in_lds(T, Lmax, wave) == ((T, Lmax) not in ((700, 130), (4000, 2)))


def test_invalid_rows_of_the_reference():
    rng = np.random.default_rng(5)
    logits = ar.grid_logits(rng, (3, 6, 4))
    labels = np.array([[0, 1], [3, 0], [1, 1]], np.int32)
    state, seg, conf, score, status = ar.align(logits, np.array([6, 6, 2]), labels, np.array([2, 2, 2]))
    assert status == 2 and np.isneginf(score[1]) and np.isneginf(score[2]) and np.isfinite(score[0])
    assert np.all(state[1:] == -1) and np.all(seg[1:] == -1) and np.all(conf[1:] == 0)


def test_host_side_contract_of_nabu_ctc_align():
    """size query and argument validation: all on the host, before any launch (no GPU needed)"""
    from nabu_amd import build, _hip
    build.build(verbose=False)
    lib = _hip.lib()
    ws = lib.nabu_ctc_align_ws_bytes
    for shape in ((0, 10, 3), (-1, 10, 3), (4, 0, 3), (4, -2, 3), (4, 10, -1)):
        assert ws(*shape) == 0, shape
    assert ws(4, 10, 0) > 0
    # what the worst route needs: a byte per (frame, state), or 64 words of 64 bits per 16 frames
    assert ws(2, 300, 130) >= 2 * 300 * 261
    assert ws(2, 4000, 2) >= 2 * 250 * 512
    one = ctypes.c_void_p(16)        # any non-null pointer: validation happens before it is touched
    big = 1 << 40

    def call(B=2, T=5, C=4, Lmax=3, logits=one, tl=one, lab=one, ll=one, state=one, seg=one, conf=one, score=one,
             status=one, w=one, wb=big):
        return lib.nabu_ctc_align(B, T, C, Lmax, logits, tl, lab, ll, state, seg, conf, score, status, w, wb, None)

    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(C=1), dict(Lmax=-1), dict(logits=None), dict(tl=None), dict(ll=None),
               dict(state=None), dict(seg=None), dict(conf=None), dict(score=None), dict(status=None), dict(w=None),
               dict(lab=None)):
        assert call(**kw) == -1, kw
    assert b'null labels' in lib.nabu_last_error()
    assert call(wb=ws(2, 5, 3) - 1) == -3 and b'workspace' in lib.nabu_last_error()
    # more frames than any route's LDS holds (the path and the frame terms: 8 bytes per frame)
    assert call(T=40000, C=2, Lmax=0) == -2
    msg = lib.nabu_last_error()
    assert b'LDS' in msg and str((2 * 40000 + 2 + 3) * 4).encode() in msg, msg
