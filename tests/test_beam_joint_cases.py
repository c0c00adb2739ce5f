"""tests/beam_joint_cases.py held to its own promises on the CPU: every committed seed leaves float64 a margin above
MARGIN, and the float64 pruning reference with ctc_weight 0 is the plain pruning reference."""
import numpy as np
import pytest

from tests import beam_joint_cases as J


@pytest.mark.parametrize('case', sorted(J.PRUNE_CASES), ids=lambda c: 'W%d-C%d' % c[:2])
def test_committed_prune_seeds_keep_their_margin(case):
    assert J.prune_gap(*case, J.PRUNE_CASES[case]) > J.MARGIN


@pytest.mark.parametrize('kind', sorted(J.SEARCH_SEEDS))
def test_committed_search_seeds_keep_their_margin(kind):
    assert J.search_margin(kind, J.SEARCH_SEEDS[kind]) > J.MARGIN


def test_the_search_case_is_exhaustive_at_its_width():
    """three steps over C = 4: 1, 3 and 9 live prefixes and the finished ones beside them — 4, 13 and 40 candidates"""
    C, n = J.SEARCH['C'], [1, 3, 9]
    assert [live * C + sum(n[:i]) for i, live in enumerate(n)] == [4, 13, 40] and J.SEARCH['W'] >= 40
    assert len(J.sequences(C, 2)) == 13


def test_joint_reference_without_ctc_weight_is_the_plain_one():
    W, C = 4, 6
    logits, delta, logprobs, lengths, finished, _ = J.prune_inputs(2, W, C, 1)
    a = J.prune_joint_reference(logits, delta, 0.0, logprobs, lengths, finished, 1.0, 0.7)
    b = J.prune_joint_reference(logits, np.zeros_like(delta), 0.0, logprobs, lengths, finished, 1.0, 0.7)
    np.testing.assert_array_equal(a['order'], b['order'])
    np.testing.assert_array_equal(a['all_lp'], b['all_lp'])
    c = J.prune_joint_reference(logits, delta, J.LAM, logprobs, lengths, finished, 1.0, 0.7)
    assert not np.array_equal(a['order'], c['order'])
