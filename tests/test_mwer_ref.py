"""The float64 restatement of the MWER objective (tests/mwer_ref.py) against central differences, its exact zeros, and
prepare on hand-written beams.  No GPU."""
import numpy as np
import pytest

from tests import mwer_ref as ref

END = 6          # C = 7: labels 0..5 and the end label


def small_case(N, seed, invalid=(), equal_errors=False):
    rng = np.random.RandomState(seed)
    B, L, C = 2, 3, 4
    rows = (N + 1) * B
    logits = rng.standard_normal((rows, L, C))
    stk_targets = rng.randint(0, C, size=(rows, L)).astype(np.int32)
    stk_len = rng.randint(1, L + 1, size=rows).astype(np.int32)
    errs = np.full(N * B, 3, np.int32) if equal_errors else rng.randint(0, 5, size=N * B).astype(np.int32)
    valid = np.ones(N * B, np.int32)
    for r in invalid:
        valid[r] = 0
    return logits, stk_targets, stk_len, errs, valid


def central_differences(logits, rest, lam, scale, h=1e-6):
    g = np.zeros_like(logits)
    flat, gf = logits.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = ref.loss_grad(logits, *rest, lam, scale, with_grad=False)[0].sum() * scale
        flat[i] = keep - h
        down = ref.loss_grad(logits, *rest, lam, scale, with_grad=False)[0].sum() * scale
        flat[i] = keep
        gf[i] = (up - down) / (2 * h)
    return g


@pytest.mark.parametrize('lam', [0.0, 0.01, 1.0])
@pytest.mark.parametrize('N,invalid,equal', [(1, (), False), (2, (), False), (4, (), False), (4, (1, 4, 6), False),
                                             (2, (0,), False), (4, (), True), (2, (), True)])
def test_gradient_matches_central_differences(N, invalid, equal, lam):
    logits, *rest = small_case(N, 11 * N + len(invalid), invalid, equal)
    scale = 0.5
    d = ref.loss_grad(logits, *rest, lam, scale)[3]
    fd = central_differences(logits, rest, lam, scale)
    assert np.abs(d - fd).max() <= 1e-8 * max(1.0, np.abs(fd).max())


def test_exact_zeros():
    N, B = 4, 2
    logits, stk_targets, stk_len, errs, valid = small_case(N, 5, invalid=(1, 4))
    stk_len[3] = 1
    d = ref.loss_grad(logits, stk_targets, stk_len, errs, valid, 0.0, 0.5)[3]
    L = logits.shape[1]
    for r in range((N + 1) * B):
        assert not d[r, stk_len[r]:].any()                 # past stk_len
    assert not d[1].any() and not d[4].any()               # rows of invalid hypotheses
    assert not d[N * B:].any()                             # the reference rows at ce_weight == 0
    assert d[:N * B].any() and L > 1
    # equal error counts over the valid slots: no hypothesis row moves, whatever the invalid ones count
    errs[:] = 3
    errs[1], errs[4] = 0, 9
    d = ref.loss_grad(logits, stk_targets, stk_len, errs, valid, 1.0, 0.5)[3]
    assert not d[:N * B].any() and d[N * B:].any()
    # N = 1: the cross-entropy term alone
    logits, stk_targets, stk_len, errs, valid = small_case(1, 6)
    loss, risk, nll_ref, d = ref.loss_grad(logits, stk_targets, stk_len, errs, valid, 1.0, 1.0)
    assert not d[:B].any()
    np.testing.assert_array_equal(risk, errs.astype(np.float64))
    np.testing.assert_allclose(loss - risk, nll_ref, rtol=1e-14)


def test_float32_switch_runs_the_same_formulas():
    logits, *rest = small_case(4, 9, invalid=(2,))
    want = ref.loss_grad(logits, *rest, 0.01, 0.5)
    got = ref.loss_grad(logits, *rest, 0.01, 0.5, dtype=np.float32)
    for g, w in zip(got, want):
        assert g.dtype == np.float32
        assert ref.rel_err(g, w) < 1e-5


def hand_written_beams():
    """B = 2, N = 4, S = 3, C = 7 (end label 6).  Utterance 0: a b | a b (the finished twin: same labels, same length) |
    the empty hypothesis | a spare slot.  Utterance 1: a hypothesis of length S | its prefix | the prefix again |
    another one of length S."""
    seq = np.array([[[1, 2, 0], [1, 2, 5], [4, 4, 4], [3, 3, 3]],
                    [[1, 2, 3], [1, 2, 0], [1, 2, 4], [1, 2, 4]]], np.int32)
    lengths = np.array([[2, 2, 0, 3], [3, 2, 2, 3]], np.int32)
    scores = np.array([[-1.0, -1.5, -2.0, -ref.FLT_MAX], [-0.5, -0.7, -0.9, -1.1]], np.float32)
    targets = np.array([[1, 2, END, 0, 0], [1, 2, 3, 4, END]], np.int32)
    target_len = np.array([3, 5], np.int32)
    return seq, lengths, scores, targets, target_len


def test_prepare_on_hand_written_beams():
    seq, lengths, scores, targets, target_len = hand_written_beams()
    stk, stk_len, hyp_len, valid = ref.prepare(seq, lengths, scores, targets, target_len, 7)
    B, N = 2, 4
    assert stk.shape == ((N + 1) * B, 5)
    row = lambda n, b: list(stk[n * B + b, :stk_len[n * B + b]])
    # utterance 0
    assert row(0, 0) == [1, 2, END] and valid[0 * B + 0] == 1
    assert row(1, 0) == [END] and valid[1 * B + 0] == 0            # the unfinished / finished pair is one target
    assert row(2, 0) == [END] and valid[2 * B + 0] == 1 and hyp_len[2 * B + 0] == 0     # length 0, a hypothesis
    assert row(3, 0) == [END] and valid[3 * B + 0] == 0            # -FLT_MAX
    # utterance 1
    assert row(0, 1) == [1, 2, 3, END] and hyp_len[0 * B + 1] == 3  # length S
    assert row(1, 1) == [1, 2, END] and valid[1 * B + 1] == 1
    assert row(2, 1) == [END] and valid[2 * B + 1] == 0            # labels past the length do not tell them apart
    assert row(3, 1) == [1, 2, 4, END] and valid[3 * B + 1] == 1
    # the reference slot
    assert row(N, 0) == [1, 2, END] and row(N, 1) == [1, 2, 3, 4, END]
    np.testing.assert_array_equal(hyp_len, [2, 3, 0, 2, 0, 0, 0, 3])
    np.testing.assert_array_equal(stk_len[:N * B], hyp_len + 1)
    assert not stk[0, 3:].any()                                    # zeros behind the end label
    e = ref.errors(stk, hyp_len, targets, target_len)
    np.testing.assert_array_equal(e.reshape(N, B), [[0, 1], [2, 2], [2, 4], [2, 1]])


def test_a_duplicate_of_a_spare_slot_stays_valid():
    seq = np.array([[[1, 2], [1, 2]]], np.int32)
    stk, stk_len, hyp_len, valid = ref.prepare(seq, [[2, 2]], [[-ref.FLT_MAX, -1.0]], [[1, END]], [2], 7)
    np.testing.assert_array_equal(valid, [0, 1])
    assert list(stk[1, :3]) == [1, 2, END]


def test_levenshtein_and_tile():
    assert ref.levenshtein([], [1, 2]) == 2 and ref.levenshtein([1, 2, 3], [1, 3]) == 1
    assert ref.levenshtein([1, 2, 3], [3, 2, 1]) == 2 and ref.levenshtein([5], [5]) == 0
    x = np.arange(6.0).reshape(2, 3)
    y = ref.tile(x, 3)
    assert y.shape == (6, 3) and (y[2:4] == x).all() and (y[4:] == x).all()
    np.testing.assert_array_equal(ref.tile_bwd(y, 3), 3 * x)
