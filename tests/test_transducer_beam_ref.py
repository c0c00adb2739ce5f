"""The float64 restatement of the transducer's beam search (tests/transducer_beam_ref.py) held to what it must equal:
the enumeration of every path (brute_force_nll) when nothing is pruned, the greedy search at W = 1, a hand-built case in
which the merge changes the winner, and the edges el = 0, el = 1, S = 1.  Also: the inputs of the GPU tests meet the
conditions those tests assert, and both entry points are declared and bound.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import transducer_beam_cases as bc
from tests import transducer_beam_ref as br
from tests import transducer_ref as tr
from tests.test_hip_transducer import _greedy_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(rng, C, S):
    """prediction logits of every label history of length <= S"""
    return {y: rng.standard_normal(C) for n in range(S + 1) for y in itertools.product(range(C - 1), repeat=n)}


@pytest.mark.parametrize('C,T,S,W', [(3, 4, 2, 8), (3, 3, 3, 16)])
def test_unpruned_search_gives_the_enumerations_posteriors(C, T, S, W):
    rng = np.random.default_rng(C * 100 + T)
    f = rng.standard_normal((1, T, C))
    tab = _table(rng, C, S)
    assert len(tab) <= W
    res = br.beam_search(f, [T], S, W, lambda b, y: tab[tuple(y)])
    finals = dict(res['finals'][0])
    assert len(res['finals'][0]) == len(finals) == len(tab)          # every sequence, once
    for y in tab:
        g = np.stack([tab[y[:u]] for u in range(len(y) + 1)])
        nll, _ = tr.brute_force_nll(f[0], g, list(y))
        assert abs(finals[y] + nll) < 1e-13, (y, finals[y], -nll)
    scores = [s for _, s in res['finals'][0]]
    assert scores == sorted(scores, reverse=True)
    assert abs(np.exp(scores).sum() - sum(np.exp(-tr.brute_force_nll(f[0], np.stack([tab[y[:u]] for u in range(len(y) + 1)]),
                                                                   list(y))[0]) for y in tab)) < 1e-13
    assert not any(t['out_len'].max() >= 0 for t in res['trace'][T + S - 1:])     # nothing active after el + S iterations


@pytest.mark.parametrize('C', [5, 70])
def test_beam_of_one_takes_the_greedy_decisions(C):
    """labels and lengths always (the planted ties included: the blank has the largest index in both); the score on
    the rows that ran out of frames.  Row 2 reaches S with frames left: there the beam pays for the blanks"""
    S = 4
    f, gtab, enc_len, blank = _greedy_inputs(C)
    T = f.shape[1]
    g_ids, g_len, g_pos, g_score, _, _ = tr.greedy_search(f, enc_len, S, lambda b, ids: gtab[b, len(ids)], T + S)
    res = br.beam_search(f, enc_len, S, 1, lambda b, y: gtab[b, len(y)])
    ids, lens, scores = br.best(res['finals'], S)
    assert np.array_equal(ids, g_ids) and np.array_equal(lens, g_len)
    out = g_pos >= np.minimum(enc_len, T)
    assert out.sum() >= 3 and not out.all()
    assert np.allclose(scores[out], g_score[out], rtol=0, atol=1e-12)
    assert np.all(scores[~out] < g_score[~out])
    assert all(len(fin) == 1 for fin in res['finals']) and res['merges'] == [0] * len(enc_len)


def _merge_case():
    """C 3, T 2, S 1: blank 3/4, label 0 at 0, label 1 at -1 on both frames; after label 0 the blank is certain"""
    f = np.tile(np.array([0.0, -1.0, 0.75]), (1, 2, 1))
    tab = {(): np.zeros(3), (0,): np.array([0.0, 0.0, 40.0]), (1,): np.zeros(3)}
    return f, tab


def test_the_merge_changes_the_winner():
    f, tab = _merge_case()
    p = np.exp(f[0, 0] - np.log(np.exp(f[0, 0]).sum()))
    first, second, empty = p[0], p[2] * p[0], p[2] * p[2]                # (0) at frame 0, (0) at frame 1, ()
    assert first < empty and second < empty < first + second
    for W in (2, 4):
        merged = br.beam_search(f, [2], 1, W, lambda b, y: tab[tuple(y)])
        plain = br.beam_search(f, [2], 1, W, lambda b, y: tab[tuple(y)], merge=False)
        assert merged['merges'] == [W // 2] and plain['merges'] == [0]                # (1) merges too when it is kept
        (y, s), (y2, s2) = merged['finals'][0][:2]
        assert y == (0,) and y2 == () and abs(np.exp(s) - (first + second)) < 1e-12 and abs(np.exp(s2) - empty) < 1e-15
        assert plain['finals'][0][0][0] == () and abs(np.exp(plain['finals'][0][0][1]) - empty) < 1e-15
        assert abs(np.exp(plain['finals'][0][1][1]) - first) < 1e-12 and plain['finals'][0][1][0] == (0,)
    both = [s for y, s in br.beam_search(f, [2], 1, 4, lambda b, y: tab[tuple(y)], merge=False)['finals'][0] if y == (0,)]
    assert len(both) == 2 and abs(np.exp(both[1]) - second) < 1e-12     # without the merge the beam holds (0) twice


def test_edges():
    rng = np.random.default_rng(7)
    C, T = 4, 3
    f = rng.standard_normal((3, T, C))
    tab = _table(rng, C, 2)
    g_fn = lambda b, y: tab[tuple(y)]                                    # noqa: E731
    res = br.beam_search(f, [0, 1, -5], 2, 3, g_fn)
    # el = 0 (and a negative length, clamped): the empty hypothesis, complete at once, and nothing active ever
    for b in (0, 2):
        assert res['finals'][b] == [((), 0.0)]
        assert all(t['out_len'][b].max() == -1 and t['fin_len'][b].tolist() == [0, -1, -1] for t in res['trace'])
    # el = 1: a hypothesis of u labels completes at iteration u; the posteriors are the enumeration's
    assert res['finals'][1][0][0] == () or res['finals'][1][0][1] >= res['finals'][1][1][1]
    for y, s in res['finals'][1]:
        g = np.stack([tab[y[:u]] for u in range(len(y) + 1)])
        assert abs(s + tr.brute_force_nll(f[1, :1], g, list(y))[0]) < 1e-13
    t0 = res['trace'][0]
    assert t0['fin_len'][1].tolist() == [0, -1, -1] and t0['out_len'][1].tolist() == [1, 1, -1]    # the beam shrank to 2
    assert t0['parent'][1].tolist() == [0, 0, 2] and t0['emit'][1].tolist() == [1, 1, 0]
    assert res['shrinks'][1] >= 1
    # S = 1: a hypothesis with one label has only its blank
    res1 = br.beam_search(f, [T, T, T], 1, 8, g_fn)
    for b in range(3):
        assert sorted(len(y) for y, _ in res1['finals'][b]) == [0, 1, 1, 1]
        for y, s in res1['finals'][b]:
            g = np.stack([tab[y[:u]] for u in range(len(y) + 1)])
            assert abs(s + tr.brute_force_nll(f[b], g, list(y))[0]) < 1e-13
    assert all(c > 0 for c in res1['capped'])


@pytest.mark.parametrize('C', [3, 5, 70])
@pytest.mark.parametrize('W', [1, 2, 4, 8])
def test_the_gpu_tests_inputs_meet_their_conditions(C, W):
    f, enc_len, g_fn = bc.beam_inputs(C)
    res = br.beam_search(f, enc_len, bc.S, W, g_fn)
    plain = br.beam_search(f, enc_len, bc.S, W, g_fn, merge=False)
    assert bc.conditions(res, plain, W) == []
    if W >= 2:
        assert res['finals'][0][0][0] == (0,) and plain['finals'][0][0][0] == ()      # the planted merge
    assert np.isnan(f[2]).all() and np.isnan(f[1, -1]).all()
    res32 = br.beam_search(f, enc_len, bc.S, W, g_fn, dtype=np.float32)               # float32 takes the same decisions
    assert all(np.array_equal(a['ids'], b['ids']) and np.array_equal(a['fin_ids'], b['fin_ids'])
               for a, b in zip(res['trace'], res32['trace']))


def test_both_entry_points_are_declared_and_bound():
    from nabu_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'nabu_hip.h')).read()
    for name in ('nabu_transducer_beam_ws_bytes', 'nabu_transducer_beam_step'):
        assert re.search(r'\b%s\s*\(' % name, hdr), '%s is not declared in include/nabu_hip.h' % name
        assert name in _hip.SIGNATURES, '%s has no ctypes signature' % name
    ret, args = _hip.SIGNATURES['nabu_transducer_beam_step']
    assert len(args) == 21
