"""The joint CTC/attention pruning step (nabu_beam_prune_joint) and the beam search with the CTC operand
(nabu_speller[_multi]_beam_search_joint) against float64 (tests/beam_joint_cases.py).

Selections are compared exactly, which float32 can be held to only where float64 leaves a margin: every case comes from
a seed with a float64 margin above 1e-3 (asserted on the CPU by tests/test_beam_joint_cases.py).  Scores are held to
2e-4 (rtol = atol), the bound of the beam-search scores in tests/test_hip_decode.py and tests/test_hip_multi_speller.py:
the joint score is the same chain of float32 cell steps, weighted, plus a CTC term whose error is two orders smaller
(tests/test_hip_ctc_prefix.py)."""
import numpy as np
import pytest
import torch

from nabu_amd import ops
from tests import beam_joint_cases as J

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCORE_BOUND = 2e-4


def t(a):
    return torch.tensor(a, device=DEV)


def run_prune(joint, logits, delta, lam, logprobs, lengths, finished, seen, temp, lpw):
    state = [t(a.copy()) for a in (logprobs, lengths, finished, seen)]
    if joint:
        out = ops.beam_prune_joint(t(logits), t(delta), lam, *state, temp, lpw)
    else:
        out = ops.beam_prune(t(logits), *state, temp, lpw)
    return list(out) + state        # pred, parent, stay, all_seen, logprobs, lengths, finished, seen


@pytest.mark.parametrize('case', sorted(J.PRUNE_CASES), ids=lambda c: 'W%d-C%d' % c[:2])
def test_prune_joint_without_weight_is_beam_prune_bit_for_bit(case):
    W, C, lpw, temp = case
    inputs = J.prune_inputs(J.PRUNE_B, W, C, J.PRUNE_CASES[case])
    logits, delta = inputs[:2]
    plain = run_prune(False, logits, None, 0.0, *inputs[2:], temp, lpw)
    for d in (delta, np.zeros_like(delta)):
        got = run_prune(True, logits, d, 0.0, *inputs[2:], temp, lpw)
        for a, b in zip(got, plain):
            assert torch.equal(a, b)


@pytest.mark.parametrize('case', sorted(J.PRUNE_CASES), ids=lambda c: 'W%d-C%d' % c[:2])
def test_prune_joint_selects_what_float64_selects(case):
    W, C, lpw, temp = case
    logits, delta, logprobs, lengths, finished, seen = J.prune_inputs(J.PRUNE_B, W, C, J.PRUNE_CASES[case])
    ref = J.prune_joint_reference(logits, delta, J.LAM, logprobs, lengths, finished, temp, lpw)
    assert ref['gap'].min() > J.MARGIN
    pred, parent, stay, all_seen, lp, ln, fin, sn = (x.cpu().numpy() for x in run_prune(
        True, logits, delta, J.LAM, logprobs, lengths, finished, seen, temp, lpw))
    order, bi = ref['order'], np.arange(J.PRUNE_B)[:, None]
    st = order >= W * C
    np.testing.assert_array_equal(pred, ref['all_ids'][bi, order])
    np.testing.assert_array_equal(stay, st.astype(np.int32))
    np.testing.assert_array_equal(parent, np.where(st, order - W * C, order // C))
    np.testing.assert_array_equal(ln, ref['all_len'][bi, order])
    np.testing.assert_array_equal(fin, (pred == C - 1).astype(np.int32))
    np.testing.assert_array_equal(sn, seen | (pred == C - 1))
    np.testing.assert_array_equal(all_seen, sn.all(1).astype(np.int32))
    np.testing.assert_allclose(lp, ref['all_lp'][bi, order], rtol=1e-5, atol=1e-5)
    assert not np.array_equal(order, J.prune_joint_reference(logits, delta, 0.0, logprobs, lengths, finished, temp,
                                                             lpw)['order'])       # the CTC term decides something


# ---------------------------------------------------------------------------------------------------------------
def device_state(attention, p):
    """the float64 parameters under the names the decoder's variables take"""
    from tests.test_hip_multi_speller import PRE, mech_names
    st = {PRE + 'dense/kernel': p['out_kernel'], PRE + 'dense/bias': p['out_bias']}
    for n, q in enumerate(p['lstm']):
        pre = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        st[pre + 'kernel'], st[pre + 'bias'] = q['kernel'], q['bias']
    for m, pm in enumerate(p['mem']):
        for k, name in mech_names(attention, m).items():
            st[name] = pm[k].reshape(pm[k].shape[0], 1, -1) if k == 'conv_kernel' else pm[k]
    return {k: v.astype(np.float32) for k, v in st.items()}


@pytest.mark.parametrize('kind', sorted(J.SEARCH_SEEDS))
def test_joint_beam_search_on_a_tiny_speller(kind):
    """B = 3, U = E = 32, Te = 7 with lengths (7, 4, 5), C = 4, three steps, W = 40: more slots than hypotheses, so the
    search is exhaustive.  Through the new entry point with weight 0: the plain search bit for bit.  With 0.3: every
    finished hypothesis scores (1 - w) log p_att + w log p_ctc in float64, beams come best first, and the best finished
    one is the arg-max over all label sequences of at most two labels."""
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    from tests.test_hip_multi_speller import NAMES, make_decoder
    c, seed = J.SEARCH, J.SEARCH_SEEDS[kind]
    attention, p, encs, enc_lens, ctc_logits = J.search_case(kind, seed)
    table = J.joint_table(kind, seed)
    assert J.search_margin(kind, seed) > J.MARGIN
    dec = make_decoder(attention, 'softmax', 1, c['U'], J.K_LOC, J.F_LOC, c['C'])
    store = vs.VariableStore(seed=0)
    state = device_state(attention, p)
    store.restore_from(state)
    enc_d = {NAMES[m]: t(e) for m, e in enumerate(encs)}
    lens = {NAMES[m]: SeqLen(l, torch.device(DEV)) for m, l in enumerate(enc_lens)}
    ctc_d = t(ctc_logits)
    with torch.no_grad(), vs.as_default(store), vs.variable_scope('Speller'):
        cell = dec.create_cell(enc_d, lens, False)
        args = (cell, list(enc_d.values()), list(lens.values()), c['W'], c['S'], 0.0, 1.0)
        plain = rnn_decoder.beam_search(*args)
        zero = rnn_decoder.beam_search(*args, ctc_logits=ctc_d, ctc_weight=0.0)
        joint = rnn_decoder.beam_search(*args, ctc_logits=ctc_d, ctc_weight=J.LAM)
    assert not store.restore and sorted(store.state_dict()) == sorted(state)      # the parameters are the case's
    flat = lambda r: list(r[:3]) + (list(r[3]) if isinstance(r[3], list) else [r[3]])
    for a, b in zip(flat(zero), flat(plain)):
        assert torch.equal(a, b)
    seqs, lengths, scores = (x.cpu().numpy() for x in joint[:3])
    steps, eos = seqs.shape[2], c['C'] - 1
    assert steps == c['S'] and np.all(np.isfinite(scores))
    assert np.all(scores[:, :-1] >= scores[:, 1:])                                # best first
    worst = 0.0
    for b in range(c['B']):
        seen, best = {}, None
        for w in range(c['W']):
            L = int(lengths[b, w])
            if L < steps and seqs[b, w, L] == eos:
                g = tuple(int(k) for k in seqs[b, w, :L])
                assert g not in seen and eos not in g
                seen[g] = float(scores[b, w])
                best = g if best is None else best
        assert sorted(seen) == sorted(table[b])                                   # all 13 finished hypotheses
        for g, got in seen.items():
            want = J.joint_score(*table[b][g])
            worst = max(worst, abs(got - want) / (1 + abs(want)))
            assert got == pytest.approx(want, rel=SCORE_BOUND, abs=SCORE_BOUND), (b, g)
        assert best == max(table[b], key=lambda g: J.joint_score(*table[b][g]))
    # and the CTC term is in the result: the plain search scores its hypotheses differently
    assert np.abs(np.sort(scores, 1) - np.sort(plain[2].cpu().numpy(), 1)).max() > 100 * SCORE_BOUND
    print('%s: largest score error / (1 + |score|) = %.3g' % (kind, worst))
