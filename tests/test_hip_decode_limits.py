"""The decode kernels (decode.hip) at their limits and on the beam they keep, not only on the best path: CTC beam search
at the widths where the W-th survivor decides the answer, at the kernel's maximum width and LDS request, on one label,
on -inf logits, on clamped lengths and on structural ties; the edit distance around its 256-thread wavefront and its
LDS limits; the pruning step on the states a search starts and ends with; the gather past its grid cap; and the sampled
step on rows wider than its LDS stage.

Every CTC case is built from a seed that tests/decode_cases.py admits on the CPU: the float64 oracle alone must leave
float32 no decision to get wrong (guard_bound), and that is asserted here again before the device is touched.  The
returned log-probability is held to lp_bound = 2 T eps32 max(1, |total|) — the bound in force; the largest
error-to-bound ratios seen on the MI355X are in LABNOTES.md section 22."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle as D
from nabu_amd import _hip, ops
from tests import decode_cases as dc
from tests import random_decoder_ref as R
from tests.test_hip_decode import check_ctc, check_prune, t

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def admit(dets, T, what, ties=False):
    for b, det in enumerate(dets):
        why = dc.inadmissible(det, T, ties)
        assert why is None, '%s, utterance %d: not admissible (%s)' % (what, b, why)


def small_valid_call():
    """after a refusal the entry point must still work"""
    logits, lens, W, _ = dc.plain_case('lengths', dc.PLAIN_CASES['lengths'])
    check_ctc(logits, lens, W, True, dc.oracle(logits, lens, W), 'after a refusal')


# ------------------------------------------------------------------------------------------------ CTC beam search
@pytest.mark.parametrize('W,C,T,seeds', dc.WIDTH_CASES, ids=['W%d' % c[0] for c in dc.WIDTH_CASES])
def test_ctc_the_last_survivor_decides(W, C, T, seeds):
    """the oracle's labelling at width W differs from the one at W - 1 and the one at W + 1: a selection that keeps
    one candidate too few or too many gives another answer"""
    logits = dc.width_case(W, C, T, seeds)
    dets = []
    for seed, x in zip(seeds, logits):
        det, below, above = dc.width_decides(x, W)
        assert det['labels'] != above, 'seed %d: width %d decides nothing against %d' % (seed, W, W + 1)
        if W > 1:
            assert det['labels'] != below, 'seed %d: width %d decides nothing against %d' % (seed, W, W - 1)
        dets.append(det)
    admit(dets, T, 'W %d seeds %r' % (W, seeds))
    check_ctc(logits, np.full(len(seeds), T, np.int32), W, True, dets, 'W-th survivor, W = %d' % W)


def test_ctc_maximum_width_and_its_refusals():
    """W = 256 = the thread count, C = 40: 98 464 bytes of LDS (above the 48 KiB that need the attribute), 10 240 keys
    per selection from frame 2.  W = 256 with C = 80 (180 544 bytes) and W = 257 are refused before any launch, and
    a valid call works after each refusal."""
    logits, lens, W, _ = dc.plain_case('max_width', dc.PLAIN_CASES['max_width'])
    assert (W, logits.shape[2]) == (256, 40) and (40 + 15 * 256 + 2 * 256 * 40 + 256) * 4 == 98464 > 48 * 1024
    dets = dc.oracle(logits, lens, W)
    admit(dets, logits.shape[1], 'max_width seed %d' % dc.PLAIN_CASES['max_width'])
    assert len(dets[0]['beam']) == 256
    check_ctc(logits, lens, W, True, dets, 'maximum width')
    wide = torch.zeros((1, 3, 80), device=DEV)
    three = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    assert (80 + 15 * 256 + 2 * 256 * 80 + 256) * 4 == 180544 > 160 * 1024
    with pytest.raises(_hip.NabuHipError, match='LDS'):
        ops.ctc_beam_search(wide, three, 256, True)
    small_valid_call()
    with pytest.raises(_hip.NabuHipError, match='beam_width'):
        ops.ctc_beam_search(wide[:, :, :5].contiguous(), three, 257, True)
    small_valid_call()


@pytest.mark.parametrize('name', ['one_label', 'lengths', 'neg_inf'])
def test_ctc_plain_cases(name):
    """one_label: C = 2, T = 9, W = 4, both merge settings.  lengths: 1, T and T + 5 (clamped: the oracle sees T
    frames).  neg_inf: label classes at -inf on some frames; a frame where only the blank is finite; a frame where
    the blank is -inf; and a frame that kills every candidate: no labels, log-probability -inf, ids all -1."""
    seed = dc.PLAIN_CASES[name]
    logits, lens, W, merges = dc.plain_case(name, seed)
    T = logits.shape[1]
    for merge in merges:
        dets = dc.oracle(logits, lens, W, merge)
        admit(dets, T, '%s seed %d merge %d' % (name, seed, merge))
        if name == 'neg_inf':
            assert dets[3]['labels'] == [] and dets[3]['total'] == -np.inf and not dets[3]['beam']
            assert all(np.isfinite(d['total']) and d['labels'] for d in dets[:3])
        ids, out_len, lp = check_ctc(logits, lens, W, merge, dets, '%s merge %d' % (name, merge))
        if name == 'neg_inf':
            assert out_len[3] == 0 and lp[3] == -np.inf and np.all(ids[3] == -1)


def test_ctc_structural_ties_at_the_threshold():
    """classes 1 and 2 share bit-identical logit columns: 'p 1' and 'p 2' tie exactly for every prefix p among
    candidates that do not; W cuts through a tied group (select_ties > 0), and the lower index must survive"""
    C, T, W, seeds = dc.TIE_CASE
    logits = np.stack([dc.tie_logits(C, T, s) for s in seeds])
    assert np.array_equal(logits[:, :, dc.TIE_A], logits[:, :, dc.TIE_B])
    lens = np.full(len(seeds), T, np.int32)
    for merge in (True, False):
        dets = dc.oracle(logits, lens, W, merge)
        for s, det in zip(seeds, dets):
            assert det['select_ties'] > 0, 'seed %d: the beam cuts through no tie' % s
        admit(dets, T, 'ties seeds %r' % (seeds,), ties=True)
        check_ctc(logits, lens, W, merge, dets, 'structural ties merge %d' % merge)


# ---------------------------------------------------------------------------------------------------- edit distance
def check_edit_distance(hyp, hl, ref, tl):
    got = ops.edit_distance(t(hyp), t(hl), t(ref), t(tl)).cpu().numpy()
    ldh, ldt = hyp.shape[1], ref.shape[1]
    want = [D.edit_distance(list(hyp[b, :np.clip(hl[b], 0, ldh)]), list(ref[b, :np.clip(tl[b], 0, ldt)]))
            for b in range(len(hl))]
    np.testing.assert_array_equal(got, want)
    return got


def test_edit_distance_around_the_wavefront_width():
    """hypotheses of 255, 256, 257 and 513 labels (one, one, two and three strides of 256 threads over a diagonal)
    against truths of 1, 2 and 300; and lengths outside [0, ld] are clamped"""
    rng = np.random.default_rng(3)
    hls, tls = (255, 256, 257, 513), (1, 2, 300)
    B = len(hls) * len(tls)
    hyp = rng.integers(0, 4, (B + 2, 513)).astype(np.int32)
    ref = rng.integers(0, 4, (B + 2, 300)).astype(np.int32)
    hl = np.array([h for h in hls for _ in tls] + [513 + 9, -3], np.int32)
    tl = np.array([n for _ in hls for n in tls] + [300 + 1, 7], np.int32)
    got = check_edit_distance(hyp, hl, ref, tl)
    assert got[-1] == 7                                      # hyp_len < 0 is an empty hypothesis


def test_edit_distance_lds_opt_in_and_refusal():
    """ldh = 4096 is the first row width whose 3 (ldh + 1) ints = 49 164 bytes exceed 48 KiB; ldh = 13 653 needs
    163 848 bytes, more than the 160 KiB of a workgroup, and is refused before any launch"""
    rng = np.random.default_rng(4)
    assert 3 * 4096 * 4 <= 48 * 1024 < 3 * 4097 * 4 == 49164 and 3 * 13653 * 4 <= 160 * 1024 < 3 * 13654 * 4
    hyp = rng.integers(0, 5, (5, 4096)).astype(np.int32)
    ref = rng.integers(0, 5, (5, 300)).astype(np.int32)
    hl = np.array([4096, 3, 0, 40, 257], np.int32)
    tl = np.array([300, 300, 5, 0, 17], np.int32)
    check_edit_distance(hyp, hl, ref, tl)
    one = np.ones(1, np.int32)
    with pytest.raises(_hip.NabuHipError, match='LDS'):
        ops.edit_distance(torch.zeros((1, 13653), dtype=torch.int32, device=DEV), t(one), t(ref[:1]), t(one))
    check_edit_distance(hyp[:, :37], np.minimum(hl, 37), ref, tl)


def test_edit_distance_without_a_hypothesis_or_a_truth_tensor():
    """ldh = 0 and ldt = 0: ops.edit_distance passes a null pointer; the distance is the other side's length"""
    rng = np.random.default_rng(5)
    full = rng.integers(0, 4, (3, 9)).astype(np.int32)
    none = np.zeros((3, 0), np.int32)
    n = np.array([9, 0, 4], np.int32)
    np.testing.assert_array_equal(check_edit_distance(none, n, full, n), n)
    np.testing.assert_array_equal(check_edit_distance(full, n, none, n), n)
    np.testing.assert_array_equal(check_edit_distance(none, n, none, n), 0)


# --------------------------------------------------------------------------------------------------------- pruning
def first_step(B, W):
    lp = np.full((B, W), -np.inf, np.float32)
    lp[:, 0] = 0.0
    z = np.zeros((B, W), np.int32)
    return lp, z, z.copy(), z.copy()


def random_state(rng, B, W, p_fin=0.3):
    finished = (rng.uniform(size=(B, W)) < p_fin).astype(np.int32)
    return (-rng.uniform(0, 5, (B, W)).astype(np.float32), rng.integers(0, 7, (B, W)).astype(np.int32), finished,
            finished.copy())


@pytest.mark.parametrize('W,C,lpw', [(16, 6, 0.0), (16, 6, 1.0), (300, 3, 0.0), (300, 3, 1.0)])
def test_beam_prune_first_step(W, C, lpw):
    """logprobs = [0, -inf, ...]: C live candidates, fewer than W; the rest of the beam is filled with the -FLT_MAX
    'stay' candidates (lpw = 0) or, where the length penalty takes those to -inf as well, with the lowest indices.
    W = 300 has more beams than the workgroup has threads (the strided prologue and epilogue)."""
    rng = np.random.default_rng(W + C)
    logits = rng.normal(0, 2, (3, W, C)).astype(np.float32)
    check_prune(logits, *first_step(3, W), 1.0, lpw)


@pytest.mark.parametrize('W,C,lpw,temp', [(1, 5, 0.0, 1.0), (1, 2, 1.0, 1.0), (100, 40, 1.0, 1.0), (100, 40, 0.0, 2.0)])
def test_beam_prune_one_beam_and_a_wide_beam(W, C, lpw, temp):
    rng = np.random.default_rng(10 * W + C)
    logits = rng.normal(0, 2, (3, W, C)).astype(np.float32)
    check_prune(logits, *random_state(rng, 3, W), temp, lpw)


@pytest.mark.parametrize('W,C,lpw', [(8, 5, 0.0), (8, 5, 1.0), (300, 3, 0.0)])
def test_beam_prune_all_beams_finished(W, C, lpw):
    """every selection is a stay, in the order of the scores, and all_seen = 1"""
    rng = np.random.default_rng(W)
    logits = rng.normal(0, 2, (2, W, C)).astype(np.float32)
    lp, lengths, finished, seen = random_state(rng, 2, W, p_fin=2.0)
    assert finished.all()
    out = check_prune(logits, lp, lengths, finished, seen, 1.0, lpw)
    assert out['stay'].all() and out['all_seen'].all()
    for b in range(2):
        assert sorted(out['parent'][b]) == list(range(W))


def test_beam_prune_stay_ties_with_an_expansion():
    """beam 1 is finished with log-probability -1.25; beam 2 has log-probability -1.25 and a row [0, -200, ...] whose
    log-softmax is exactly [0, -200, ...] (exp(-200) is 0 in float32), so its class-0 expansion scores -1.25 + 0:
    bit-equal to the stay of beam 1.  The expansion has the lower index and goes first — in utterance 0 both are
    selected (their order shows); in utterance 1 three candidates lie above them (-0.2 and twice -0.1 - ln 2) and they
    compete for the last slot (the expansion alone survives)."""
    W, C = 4, 5
    rng = np.random.default_rng(12)
    logits = rng.normal(0, 1, (2, W, C)).astype(np.float32)
    logits[:, 2] = -200.0
    logits[:, 2, 0] = 0.0
    logits[1, 0], logits[1, 3] = (0.0, 0.0, -200.0, -200.0, -200.0), (-200.0, 0.0, -200.0, -200.0, -200.0)
    lp = np.array([[-9.0, -1.25, -1.25, -9.5], [-0.1, -1.25, -1.25, -0.2]], np.float32)
    lengths = np.zeros((2, W), np.int32)
    finished = np.array([[0, 1, 0, 0]] * 2, np.int32)
    ref = check_prune(logits, lp, lengths, finished, finished.copy(), 1.0, 0.0, want_only=True)
    assert np.all(ref['all_lp'][:, 2 * C] == ref['all_lp'][:, W * C + 1])          # bit-equal in float32
    assert list(ref['order'][0, :2]) == [2 * C, W * C + 1]
    assert list(ref['order'][1]) == [3 * C + 1, 0, 1, 2 * C]
    check_prune(logits, lp, lengths, finished, finished.copy(), 1.0, 0.0)


def test_beam_prune_length_penalty_on_empty_hypotheses():
    """lpw = 0.7 with every length 0: penalties (5/6)^0.7 and 1"""
    rng = np.random.default_rng(13)
    W, C = 8, 5
    logits = rng.normal(0, 2, (3, W, C)).astype(np.float32)
    lp, _, finished, seen = random_state(rng, 3, W)
    check_prune(logits, lp, np.zeros((3, W), np.int32), finished, seen, 1.0, 0.7)


def test_beam_prune_a_nan_utterance_among_healthy_ones():
    """utterance 1 has NaN logits and, in its finished beams, NaN log-probabilities: fewer than W candidates can be
    compared, and the remaining slots are filled with whatever index the round has (g.i == INT_MAX).  The call
    returns, that utterance's parent and stay are in range, and the healthy utterances are untouched by it."""
    rng = np.random.default_rng(14)
    B, W, C = 3, 8, 5
    logits = rng.normal(0, 2, (B, W, C)).astype(np.float32)
    lp, lengths, finished, seen = random_state(rng, B, W)
    logits[1] = np.nan
    finished[1] = seen[1] = np.arange(W) % 2
    lp[1, 1::2] = np.nan
    got = check_prune(logits, lp, lengths, finished, seen, 1.0, 0.0, rows=[0, 2])
    assert np.all((got['parent'][1] >= 0) & (got['parent'][1] < W)) and np.all(np.isin(got['stay'][1], (0, 1)))


@pytest.mark.parametrize('F', [1, 1025, 64 * 1024 + 3])
def test_beam_gather_rows_past_the_grid_cap(F):
    """a row of F floats takes ceil(F / 1024) blocks in y, capped at 64: F = 64 * 1024 + 3 is strided"""
    rng = np.random.default_rng(F)
    B, W = 2, 3
    fresh = rng.normal(size=(B, W, F)).astype(np.float32)
    old = rng.normal(size=(B, W, F)).astype(np.float32)
    parent = np.array([[2, 0, 0], [1, 1, 2]], np.int32)
    stay = np.array([[0, 1, 0], [1, 0, 1]], np.int32)
    got = ops.beam_gather(t(fresh), t(old), t(parent), t(stay)).cpu().numpy()
    bi = np.arange(B)[:, None]
    np.testing.assert_array_equal(got, np.where(stay[:, :, None] > 0, old[bi, parent], fresh[bi, parent]))


# -------------------------------------------------------------------------------------------------------- sampling
def sample_steps(rows):
    """rows: list of [B, C] float32 logits, one per step -> (next_ids per step, nll, lengths)"""
    B, S = rows[0].shape[0], len(rows)
    seq = torch.zeros((B, S), dtype=torch.int32, device=DEV)
    lengths, finished = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(2))
    nll = torch.zeros(B, dtype=torch.float32, device=DEV)
    ids = [ops.sample_advance(t(lg), 77, 9000 + s, s, seq, lengths, finished, nll)[0].cpu().numpy()
           for s, lg in enumerate(rows)]
    return ids, nll.cpu().numpy(), lengths.cpu().numpy()


@pytest.mark.parametrize('C', [4096, 4097])
def test_sample_step_nll_on_wide_rows(C):
    """C = 4096 is the widest row staged in LDS, C = 4097 the first one walked in place: nll against the float64 sum
    of logsumexp - logit over the ids the kernel drew, to the 1e-6 relative of test_step_nll_against_float64"""
    B, S = 5, 3
    rng = np.random.default_rng(C)
    rows = [(2.0 * rng.normal(size=(B, C))).astype(np.float32) for _ in range(S)]
    ids, nll, lengths = sample_steps(rows)
    ref = R.State(B, S)
    for s, lg in enumerate(rows):
        assert np.all((ids[s] >= 0) & (ids[s] < C))
        ref.advance(s, lg, ids[s])
    np.testing.assert_array_equal(lengths, ref.lengths)
    rel = np.abs(nll - ref.nll) / ref.nll
    print('C = %d: nll against float64, largest relative error %.3g' % (C, rel.max()))
    assert ref.nll.min() > 0 and rel.max() < 1e-6


def test_sample_step_in_place_walk_equals_the_staged_one():
    """4096-wide rows whose last two classes are -inf, and the same rows with one more -inf class: the extra term adds
    an exact zero to one lane's partial sum and to the draw's running sums, nothing else differs — next_ids and nll
    must be bit-identical between the staged (4096) and the in-place (4097) path"""
    B, S, C = 5, 3, 4096
    rng = np.random.default_rng(41)
    rows = [(2.0 * rng.normal(size=(B, C))).astype(np.float32) for _ in range(S)]
    for lg in rows:
        lg[:, -2:] = -np.inf
    wider = [np.concatenate([lg, np.full((B, 1), -np.inf, np.float32)], 1) for lg in rows]
    ids_a, nll_a, len_a = sample_steps(rows)
    ids_b, nll_b, len_b = sample_steps(wider)
    np.testing.assert_array_equal(np.stack(ids_a), np.stack(ids_b))
    assert nll_a.tobytes() == nll_b.tobytes() and np.all(nll_a > 0)
    np.testing.assert_array_equal(len_a, len_b)
