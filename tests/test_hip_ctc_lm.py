"""The CTC beam search with a label n-gram (nabu_ctc_beam_search_lm) against its float64 reference
(tests/ctc_lm_ref.py) on the cases of tests/ctc_lm_cases.py.

Labellings are compared exactly, which float32 can be held to only where the reference leaves margins above
decode_cases.guard_bound: every case comes from a committed seed (asserted on the CPU by tests/test_ctc_lm_cases.py, and
here again before the device is touched).  The returned log-probability is held to decode_cases.lp_bound scaled by
(1 + alpha): the total of the plain search's bound, plus the LM terms, whose sum is alpha times a number of the size of
the total and is accumulated in the same float32 chain."""
import numpy as np
import pytest
import torch

from nabu_amd import ops
from tests import ctc_lm_cases as CC
from tests import ctc_lm_ref as R
from tests import decode_cases as DC
from tests import ngram_lm_ref as NR

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def t(a):
    return torch.tensor(a, device=DEV)


def run(logits, lens, table, order, alpha, beta, W, merge):
    ids, out_len, lp = ops.ctc_beam_search_lm(t(logits), t(lens), t(table), order, alpha, beta, W, merge)
    return ids.cpu().numpy(), out_len.cpu().numpy(), lp.cpu().numpy()


def check(got, dets, lens, T, alpha):
    """ids, lengths exactly; log-probabilities within lp_bound * (1 + alpha)"""
    ids, out_len, lp = got
    want_ids = np.full(ids.shape, -1, np.int32)
    for b, d in enumerate(dets):
        want_ids[b, :len(d['labels'])] = d['labels']
    np.testing.assert_array_equal(out_len, [len(d['labels']) for d in dets])
    np.testing.assert_array_equal(ids, want_ids)
    for b, d in enumerate(dets):
        n = max(1, int(np.clip(lens[b], 0, T)))
        bound = DC.lp_bound(n, d['total']) * (1.0 + alpha)
        print('utterance %d: |lp - reference| = %.3g, bound %.3g' % (b, abs(lp[b] - d['total']), bound))
        assert abs(lp[b] - d['total']) <= bound, (b, lp[b], d['total'], bound)


@pytest.mark.parametrize('name,order', CC.IDENTITY)
def test_without_weights_it_is_ctc_beam_search_bit_for_bit(name, order):
    logits, lens, W, merges = DC.plain_case(name, DC.PLAIN_CASES[name])
    table = t(NR.random_table(logits.shape[2], order, 3))
    for merge in merges:
        plain = ops.ctc_beam_search(t(logits), t(lens), W, merge)
        fused = ops.ctc_beam_search_lm(t(logits), t(lens), table, order, 0.0, 0.0, W, merge)
        for a, b in zip(fused, plain):
            assert torch.equal(a, b)
        assert torch.equal(fused[2].view(torch.int32), plain[2].view(torch.int32))


@pytest.mark.parametrize('case', CC.PARITY, ids=lambda c: c[0])
def test_parity_with_the_float64_reference(case):
    name, B, T, C, lens, W, order, merge = case
    seed = CC.PARITY_SEEDS[name]
    dets = CC.parity_reference(case, seed)
    assert CC.admissible(dets, lens, T)                          # before the device is touched
    logits, lens, table = CC.parity_case(case, seed)
    check(run(logits, lens, table, order, CC.ALPHA, CC.BETA, W, merge), dets, lens, T, CC.ALPHA)


@pytest.mark.parametrize('name', sorted(CC.SELF_PATHS))
def test_no_term_on_the_self_loop(name):
    """the winner holds label 0 over several frames; a search that added the term on the repeated-label self loop would
    return another labelling (the reference's wrong variant decides that)"""
    seed = CC.SELF_SEEDS[name]
    assert CC.self_loop_ok(name, seed)
    det, wrong = CC.self_loop_reference(name, seed)
    logits, lens, table, merge = CC.self_loop_case(name, seed)
    got = run(logits, lens, table, 2, CC.SELF_ALPHA, 0.0, CC.SELF_W, merge)
    check(got, [det], lens, logits.shape[1], CC.SELF_ALPHA)
    assert list(got[0][0, :got[1][0]]) != wrong['labels']


def test_the_lm_changes_the_winner():
    m, seed = CC.MATTERS, CC.MATTERS_SEED
    assert CC.matters_ok(seed)
    fused, plain = CC.matters_reference(seed)
    logits, lens, table = CC.matters_case(seed)
    got = run(logits, lens, table, m['order'], m['alpha'], m['beta'], m['W'], True)
    check(got, fused, lens, m['T'], m['alpha'])
    ids, out_len, _ = (x.cpu().numpy() for x in ops.ctc_beam_search(t(logits), t(lens), m['W'], True))
    for b in range(m['B']):
        assert list(ids[b, :out_len[b]]) == plain[b]['labels'] != fused[b]['labels']


def test_argument_errors():
    from nabu_amd import _hip
    logits, lens = t(np.zeros((1, 3, 4), np.float32)), t(np.array([3], np.int32))
    table = t(np.zeros((4, 4), np.float32))
    with pytest.raises(_hip.NabuHipError, match='at least 1'):
        ops.ctc_beam_search_lm(logits, lens, table, 0, 1.0)
    with pytest.raises(_hip.NabuHipError, match='shape'):
        ops.ctc_beam_search_lm(logits, lens, table, 3, 1.0)
    with pytest.raises(_hip.NabuHipError, match='2\\^24'):
        ops.ctc_beam_search_lm(logits, lens, table, 13, 1.0)
    for alpha, beta in ((-1.0, 0.0), (float('nan'), 0.0), (1.0, float('inf'))):
        with pytest.raises(_hip.NabuHipError, match='lm_weight|insertion_bonus'):
            ops.ctc_beam_search_lm(logits, lens, table, 2, alpha, beta)
    lib = _hip.lib()
    one = 16
    assert lib.nabu_ctc_beam_search_lm(1, 3, 4, 4, 1, one, one, one, 0, 1.0, 0.0, one, one, None, one, 1 << 30, None) == -1
    assert lib.nabu_ctc_beam_search_lm(1, 3, 41, 4, 1, one, one, one, 5, 1.0, 0.0, one, one, None, one, 1 << 30, None) == -2
    assert b'2^24' in lib.nabu_last_error()
    assert lib.nabu_ctc_beam_lm_ws_bytes(32, 125, 40, 100) == 32 * (1 + 125 * 100) * (5 + 39) * 4
