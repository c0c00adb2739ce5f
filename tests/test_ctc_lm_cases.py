"""CPU: the float64 reference of the CTC beam search with a label n-gram (tests/ctc_lm_ref.py) against the oracle it
extends and against exhaustive enumeration, and the admissibility of every committed seed of tests/ctc_lm_cases.py."""
import itertools

import numpy as np
import pytest

from oracle import decode_oracle as D
from tests import ctc_lm_cases as CC
from tests import ctc_lm_ref as R
from tests import decode_cases as DC
from tests import ngram_lm_ref as NR

KEYS = ('labels', 'select_gap', 'select_ties', 'order_gap', 'top_gap', 'max_abs_total')


@pytest.mark.parametrize('name', sorted(DC.PLAIN_CASES))
def test_without_weights_it_is_the_oracle(name):
    """alpha = beta = 0 on committed seeds of decode_cases: the labelling, the total, the final beam and every margin of
    oracle.decode_oracle.ctc_beam_search"""
    logits, lens, W, merges = DC.plain_case(name, DC.PLAIN_CASES[name])
    W = min(W, 32)                                   # (max_width: 256 is the kernel's limit, not the reference's)
    C = logits.shape[2]
    table = NR.random_table(C, 2, 0)
    for merge in merges:
        want = D.ctc_decode_batch(logits, np.clip(lens, 0, logits.shape[1]), W, merge, details=True)
        got = R.search_batch(logits, lens, table, 2, 0.0, 0.0, W, merge)
        for g, w in zip(got, want):
            for k in KEYS:
                assert g[k] == w[k], (name, k)
            assert g['total'] == w['total'] or (np.isneginf(g['total']) and np.isneginf(w['total']))
            assert [b[0] for b in g['beam']] == [b[0] for b in w['beam']]


def test_width_cases_without_weights_are_the_oracle():
    W, C, T, seeds = DC.WIDTH_CASES[2]
    for x in DC.width_case(W, C, T, seeds):
        want = D.ctc_beam_search(x, W, True, details=True)
        got = R.search(x, NR.random_table(C, 3, 1), 3, 0.0, 0.0, W, True, details=True)
        assert all(got[k] == want[k] for k in KEYS) and got['total'] == want['total']


@pytest.mark.parametrize('seed', range(20))
def test_a_full_beam_scores_every_labelling_exactly(seed):
    """C = 3, T = 4, order 2, W = 64 (every prefix fits): for every labelling l in the final beam,
    fused total = log P_ctc(l) + alpha log P_lm(l . eos) + beta |l|, the CTC term by enumeration of all C^T paths"""
    C, T, order, alpha, beta = 3, 4, 2, 0.7, 0.4
    rng = np.random.default_rng([seed, 3])
    logits = rng.standard_normal((T, C))
    table = NR.random_table(C, order, seed)
    det = R.search(logits, table, order, alpha, beta, 64, False, details=True)
    seen = {tuple(g): v for g, v in det['beam']}
    every = [g for n in range(T + 1) for g in itertools.product(range(C - 1), repeat=n)]
    worst = 0.0
    for g in every:
        ctc = D.ctc_label_prob_bruteforce(logits, list(g))
        if ctc == -np.inf:
            assert g not in seen
            continue
        want = ctc + alpha * NR.sequence_logprob(table.astype(np.float64), g, C, order) + beta * len(g)
        worst = max(worst, abs(seen[g] - want))
    assert len(seen) == sum(1 for g in every if D.ctc_label_prob_bruteforce(logits, list(g)) > -np.inf)
    assert worst < 1e-12, worst
    assert det['total'] == max(seen.values())


@pytest.mark.parametrize('case', CC.PARITY, ids=lambda c: c[0])
def test_parity_seeds_are_admissible(case):
    assert CC.parity_ok(case, CC.PARITY_SEEDS[case[0]])


def test_parity_cases_cover_what_they_are_for():
    small = CC.parity_reference(CC.PARITY[0], CC.PARITY_SEEDS[CC.PARITY[0][0]])
    assert small[2]['labels'] == [] and small[2]['beam'] == [([], pytest.approx(small[2]['total']))]      # length 0: the root
    table = CC.parity_case(CC.PARITY[0], 0)[2]
    assert small[2]['total'] == pytest.approx(CC.ALPHA * float(table[0, 4]))                                # its end term
    # merge_repeated changes an output somewhere, the LM changes a labelling somewhere
    by_name = {c[0]: c for c in CC.PARITY}
    labels = lambda n: [d['labels'] for d in CC.parity_reference(by_name[n], CC.PARITY_SEEDS[n])]
    assert any(labels('small-W%d-n%d-merge' % (w, n)) != labels('small-W%d-n%d-keep' % (w, n))
               for w in (1, 4, 100) for n in (1, 2, 3))
    logits, lens, tab = CC.parity_case(by_name['recipe'], CC.PARITY_SEEDS['recipe'])
    plain = R.search_batch(logits, lens, tab, 3, 0.0, 0.0, 100, True)
    assert [d['labels'] for d in plain] != labels('recipe')


@pytest.mark.parametrize('name', sorted(CC.SELF_PATHS))
def test_self_loop_seeds_are_admissible_and_the_wrong_variant_picks_another_winner(name):
    assert CC.self_loop_ok(name, CC.SELF_SEEDS[name])
    det, wrong = CC.self_loop_reference(name, CC.SELF_SEEDS[name])
    assert det['labels'] != wrong['labels']


def test_lm_matters_seed_is_admissible():
    assert CC.matters_ok(CC.MATTERS_SEED)
