"""tests/transducer_align_ref.py held to an enumeration of every monotone path, and the properties of its cases that the
GPU tests (tests/test_hip_transducer_align.py) rely on.  No GPU."""
import numpy as np
import pytest

from tests import transducer_align_check as ck
from tests import transducer_align_ref as ar
from tests import transducer_cases as tc

TINY = [(T, U) for T in range(1, 6) for U in range(0, 5)]


def _quarter_terms(rng, T, U):
    """lb, ly drawn directly as multiples of 0.25: every path sum is exact, ties are genuine"""
    lb = -(rng.integers(0, 4, (T, U + 1)) / 4.0)
    ly = -(rng.integers(0, 4, (T, U + 1)) / 4.0)
    ly[:, U] = ar.NEG
    return lb, ly


@pytest.mark.parametrize('T,U', TINY)
def test_viterbi_against_every_path_with_ties(T, U):
    """quarter-valued terms: the best enumerated value IS the recursion's, and among the tied best paths the
    restatement returns the one the tie rule names; in float32 the same"""
    rng = np.random.default_rng(1000 * T + U)
    tied = 0
    for _ in range(20):
        lb, ly = _quarter_terms(rng, T, U)
        best, arg, count = ar.best_paths(lb, ly)
        for dt in (np.float64, np.float32):
            v, move, _ = ar.viterbi(lb.astype(dt), ly.astype(dt))
            state, frame = ar.backtrace(move)
            assert float(v[T - 1, U] + lb[T - 1, U]) == float(best)
            assert tuple(int(x) for x in frame) in arg
            assert tuple(int(x) for x in frame) == ar.tie_rule_choice(arg)
            assert not ar.check_path(state, frame, T, U, T, U)
        tied += len(arg) > 1
    if T >= 2 and U >= 1 and count >= 4:
        assert tied, 'no draw had tied best paths: the tie rule was not exercised'


@pytest.mark.parametrize('T,U', [(3, 2), (5, 4), (4, 3), (1, 4), (5, 0)])
def test_viterbi_against_every_path_continuous(T, U):
    """real logits through terms(): the value within rounding of the enumeration's, the path the enumerated best"""
    rng = np.random.default_rng(77 + 10 * T + U)
    C = 6
    f = (2 * rng.standard_normal((T, C))).astype(np.float32)
    g = (2 * rng.standard_normal((U + 1, C))).astype(np.float32)
    lab = rng.integers(0, C - 1, U)
    lb, ly = ar.terms(f, g, lab)
    assert np.all(lb < 0) and np.all(ly[:, :U] < 0) and np.all(ly[:, U] == ar.NEG)
    best, arg, _ = ar.best_paths(lb, ly)
    v, move, _ = ar.viterbi(lb, ly)
    state, frame = ar.backtrace(move)
    assert abs(float(v[T - 1, U] + lb[T - 1, U]) - float(best)) <= 1e-12 * abs(float(best))
    assert len(arg) == 1 and tuple(int(x) for x in frame) == arg[0]
    x, conf = ar.path_terms(lb, ly, frame)
    assert len(x) == T + U and abs(x.sum() - float(best)) <= 1e-12 * abs(float(best))
    assert np.array_equal(conf, ly[frame, np.arange(U)])


def test_align_follows_the_loss_on_rejected_rows():
    f, g, enc_len, labels, label_len = ar.grid_case((4, 6, 5, 3))
    labels = labels.copy()
    enc_len, label_len = enc_len.copy(), np.array([3, 2, 3, 1], np.int32)
    labels[1, 0] = 4                       # the blank as a label
    enc_len[2] = 0
    state, frame, conf, score, status, _ = ar.align(f, g, enc_len, labels, label_len)
    assert status == 2
    for b in (1, 2):
        assert np.isneginf(score[b]) and np.all(state[b] == -1) and np.all(frame[b] == -1) and np.all(conf[b] == 0)
    for b in (0, 3):
        assert np.isfinite(score[b]) and not ar.check_path(state[b], frame[b], enc_len[b], label_len[b], 6, 3)


@pytest.mark.parametrize('shape', ck.GRID_SHAPES, ids=ck.shape_id)
def test_grid_is_exact_and_meets_ties(shape):
    """on the grid the float32 and float64 restatements return the same path and score, every lb / ly is a multiple of
    0.25, and every case meets at least one tie at a node with both predecessors: a case without one pins nothing"""
    case = ck.grid_reference(shape)
    f, g, enc_len, labels, label_len = case.inputs
    r64, r32 = case.ref64, case.ref32
    assert r64[4] == 0 == r32[4]
    assert np.array_equal(r64[0], r32[0]) and np.array_equal(r64[1], r32[1])
    assert np.array_equal(r64[2], r32[2].astype(np.float64)) and np.array_equal(r64[3], r32[3].astype(np.float64))
    assert np.all(r64[3] * 4 == np.round(r64[3] * 4))
    if shape[1] >= 2 and shape[3] >= 1:
        assert r64[5].sum() >= 1, 'no tie on this case'
    else:                                  # one frame: no node has both predecessors, every utterance has ONE path
        assert shape == (2, 1, 3, 2)
    for b in range(shape[0]):
        assert not ar.check_path(r64[0][b], r64[1][b], enc_len[b], label_len[b], shape[1], shape[3])


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_non_finite_terms_keep_the_path_inside_the_lattice(dt):
    """a blank logit of -inf (a masked blank, a diverged model) makes lb = -inf, below the finite -1e30 that stands for
    a move that does not exist: the back-pointers must not name that move.  Column 0 never takes the label move, frame
    0 never the blank move; the path is valid, and the sum of its terms — the kernel's score — is -inf where it passes
    a -inf term"""
    rng = np.random.default_rng(3)
    T, C, Lmax = 6, 4, 3
    f = rng.standard_normal((3, T, C)).astype(np.float32)
    g = rng.standard_normal((3, Lmax + 1, C)).astype(np.float32)
    f[0, 0, C - 1] = -np.inf               # utterance 0 (no labels): the blank of node (0,0)
    f[1, :, C - 1] = -np.inf               # utterance 1: the blank of every frame
    labels = rng.integers(0, C - 1, (3, Lmax)).astype(np.int32)
    f[2, 0, labels[2, 0]] = -np.inf        # utterance 2: its first label at frame 0
    enc_len, label_len = np.array([T, T, T], np.int32), np.array([0, Lmax, Lmax], np.int32)
    with np.errstate(all='ignore'):
        state, frame, conf, score, status, _ = ar.align(f, g, enc_len, labels, label_len, dt)
    assert status == 0
    for b in range(3):
        assert not ar.check_path(state[b], frame[b], enc_len[b], label_len[b], T, Lmax), b
    sums = []
    for b in range(3):
        lb, ly = ar.terms(f[b], g[b, :label_len[b] + 1], labels[b, :label_len[b]], dt)
        sums.append(ar.path_terms(lb, ly, frame[b, :label_len[b]])[0].sum())
    assert np.isneginf(sums[0]) and np.isneginf(sums[1]) and np.isfinite(sums[2]) and frame[2, 0] >= 1
    assert np.isfinite(score[2]) and abs(float(score[2]) - float(sums[2])) <= 1e-5 * abs(float(sums[2]))
    # terms given directly: every blank of column 0 and every label of frame 0 at -inf, and NaN everywhere
    for fill in (-np.inf, np.nan):
        lb, ly = np.full((4, 3), -1.0, dt), np.full((4, 3), -1.0, dt)
        lb[:, 0], ly[0, :] = fill, fill
        ly[:, 2] = ar.NEG
        with np.errstate(all='ignore'):
            v, move, _ = ar.viterbi(lb, ly)
        assert not move[:, 0].any() and move[0, 1:].all()
        st, fr = ar.backtrace(move)
        assert not ar.check_path(st, fr, 4, 2, 4, 2)
        lb[:], ly[:] = fill, fill
        with np.errstate(all='ignore'):
            st, fr = ar.backtrace(ar.viterbi(lb, ly)[1])
        assert not ar.check_path(st, fr, 4, 2, 4, 2)


def test_constant_lattice_puts_every_label_at_frame_zero():
    f, g, enc_len, labels, label_len = ar.constant_case(3, 9, 5, 4)
    for dt in (np.float64, np.float32):
        state, frame, conf, score, status, ties = ar.align(f, g, enc_len, labels, label_len, dt)
        assert status == 0
        for b in range(3):
            Tb, Ub = int(enc_len[b]), int(label_len[b])
            assert np.all(frame[b, :Ub] == 0) and np.all(state[b, :Tb] == Ub)
            assert np.allclose(score[b], -(Tb + Ub) * np.log(5.0))
            if Tb >= 2 and Ub >= 1:
                assert ties[b] == (Tb - 1) * Ub            # every node with both predecessors ties


def test_check_path_rejects_what_is_not_a_path():
    good_state, good_frame = np.array([0, 2, 2, 3, -1], np.int32), np.array([1, 1, 3, -1], np.int32)
    assert not ar.check_path(good_state, good_frame, 4, 3, 5, 4)
    assert ar.check_path(np.array([0, 2, 1, 3, -1]), good_frame, 4, 3, 5, 4)
    assert ar.check_path(np.array([0, 2, 2, 2, -1]), good_frame, 4, 3, 5, 4)
    assert ar.check_path(good_state, np.array([1, 2, 3, -1]), 4, 3, 5, 4)
    assert ar.check_path(np.array([0, 2, 2, 3, 3]), good_frame, 4, 3, 5, 4)


def test_grid_shapes_are_the_loss_shapes_with_a_spare_class():
    assert ck.GRID_SHAPES == [s for s in tc.ALL_SHAPES if s[2] >= 3]
    assert len(ck.GRID_SHAPES) == len(tc.ALL_SHAPES) - 1
