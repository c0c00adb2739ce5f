"""CPU: every committed seed of tests/beam_lm_cases.py leaves float32 a margin above MARGIN, and the float64 prune
reference with the LM term reduces to the one of tests/beam_joint_cases.py without it."""
import numpy as np
import pytest

from tests import beam_joint_cases as J
from tests import beam_lm_cases as BC


@pytest.mark.parametrize('key', BC.PRUNE_KEYS, ids=BC.prune_id)
def test_prune_seeds_are_admissible(key):
    seed = BC.PRUNE_SEEDS[BC.prune_id(key)]
    assert BC.prune_ok(key, seed)
    (W, C, _, _), _, order, mix = key
    _, _, _, ctx, _, lengths, finished, _ = BC.prune_inputs(key, seed)
    assert lengths.min() >= order                                  # hypotheses longer than n-1: the context wraps
    assert (finished.all(), (finished == 0).all()) == (mix == 'finished', mix == 'live')
    if mix == 'both':
        assert np.all(finished.any(1) & (finished == 0).any(1))
    ref = BC.prune_reference(key, seed)
    assert ref['ctx_out'].min() >= 0 and ref['ctx_out'].max() < C ** (order - 1)


@pytest.mark.parametrize('key', [k for k in BC.PRUNE_KEYS if k[1]][:6], ids=BC.prune_id)
def test_without_the_lm_weight_the_reference_is_the_joint_one(key):
    (W, C, lpw, temp), _, order, _ = key
    logits, delta, table, ctx, logprobs, lengths, finished, _ = BC.prune_inputs(key, 0)
    got = BC.prune_lm_reference(logits, delta, BC.LAM, table, order, 0.0, ctx, logprobs, lengths, finished, temp, lpw)
    want = J.prune_joint_reference(logits, delta, BC.LAM, logprobs, lengths, finished, temp, lpw)
    for k in ('all_lp', 'all_ids', 'all_len', 'order', 'gap'):
        np.testing.assert_array_equal(got[k], want[k])


@pytest.mark.parametrize('kind', BC.SEARCH_KINDS)
def test_search_seeds_are_admissible_and_the_lm_term_decides_a_winner(kind):
    seed = BC.SEARCH_SEEDS[kind]
    assert BC.search_ok(kind, seed)
    changed = 0
    for lam in BC.SEARCH_LAMS:
        for table in BC.lm_table(kind, seed):
            fused = max(table, key=lambda g: BC.fused_score(*table[g], lam))
            plain = max(table, key=lambda g: BC.fused_score(*table[g], lam, gamma=0.0))
            changed += fused != plain
    assert changed > 0
