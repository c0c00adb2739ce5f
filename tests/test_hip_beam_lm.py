"""The pruning step with the label n-gram term (nabu_beam_prune_lm) and the attention beam search with a language model
(nabu_speller[_multi]_beam_search_ex) against float64 (tests/beam_lm_cases.py).

Selections — the survivors' contexts included — are compared exactly, which float32 can be held to only where float64
leaves a margin: every case comes from a seed with a float64 margin above 1e-3 (asserted on the CPU by
tests/test_beam_lm_cases.py and here before the device is touched).  Log-probabilities of the prune are held to the
tolerance tests/test_hip_beam_joint.py uses for the joint prune (1e-5, rtol = atol), the scores of the search to its
2e-4: the LM term is one table entry and one fused multiply-add per candidate."""
import numpy as np
import pytest
import torch

from nabu_amd import ops
from tests import beam_joint_cases as J
from tests import beam_lm_cases as BC
from tests.test_hip_beam_joint import SCORE_BOUND, device_state

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def t(a):
    return torch.tensor(a, device=DEV)


def run_lm(logits, delta, lam, table, order, gamma, ctx, logprobs, lengths, finished, seen, temp, lpw):
    state = [t(a.copy()) for a in (logprobs, lengths, finished, seen)]
    ctx_d = t(ctx.copy())
    out = ops.beam_prune_lm(t(logits), None if delta is None else t(delta), lam, t(table), order, gamma, ctx_d, *state,
                            temp, lpw)
    assert torch.equal(ctx_d, t(ctx))                     # the contexts before the step are not touched
    return list(out[:4]) + state + [out[4]]             # pred, parent, stay, all_seen, logprobs, lengths, finished, seen, ctx


@pytest.mark.parametrize('key', BC.PRUNE_KEYS, ids=BC.prune_id)
def test_prune_lm_selects_what_float64_selects(key):
    (W, C, lpw, temp), with_delta, order, mix = key
    seed = BC.PRUNE_SEEDS[BC.prune_id(key)]
    assert BC.prune_ok(key, seed)
    logits, delta, table, ctx, logprobs, lengths, finished, seen = BC.prune_inputs(key, seed)
    ref = BC.prune_lm_reference(logits, delta, BC.LAM, table, order, BC.GAMMA, ctx, logprobs, lengths, finished, temp, lpw)
    pred, parent, stay, all_seen, lp, ln, fin, sn, ctx_out = (x.cpu().numpy() for x in run_lm(
        logits, delta, BC.LAM, table, order, BC.GAMMA, ctx, logprobs, lengths, finished, seen, temp, lpw))
    sel, bi = ref['order'], np.arange(J.PRUNE_B)[:, None]
    st = sel >= W * C
    np.testing.assert_array_equal(pred, ref['all_ids'][bi, sel])
    np.testing.assert_array_equal(stay, st.astype(np.int32))
    np.testing.assert_array_equal(parent, np.where(st, sel - W * C, sel // C))
    np.testing.assert_array_equal(ctx_out, ref['ctx_out'])
    np.testing.assert_array_equal(ln, ref['all_len'][bi, sel])
    np.testing.assert_array_equal(fin, (pred == C - 1).astype(np.int32))
    np.testing.assert_array_equal(sn, seen | (pred == C - 1))
    np.testing.assert_array_equal(all_seen, sn.all(1).astype(np.int32))
    np.testing.assert_allclose(lp, ref['all_lp'][bi, sel], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('key', BC.PRUNE_KEYS, ids=BC.prune_id)
def test_prune_lm_without_weight_is_the_prune_without_lm_bit_for_bit(key):
    """gamma = 0: nabu_beam_prune_joint (with delta), and with lambda = 0 as well, or without delta: nabu_beam_prune"""
    (W, C, lpw, temp), with_delta, order, mix = key
    logits, delta, table, ctx, logprobs, lengths, finished, seen = BC.prune_inputs(key, BC.PRUNE_SEEDS[BC.prune_id(key)])

    def plain(joint, lam):
        state = [t(a.copy()) for a in (logprobs, lengths, finished, seen)]
        if joint:
            out = ops.beam_prune_joint(t(logits), t(delta), lam, *state, temp, lpw)
        else:
            out = ops.beam_prune(t(logits), *state, temp, lpw)
        return list(out) + state

    def same(lam, want):
        got = run_lm(logits, delta, lam, table, order, 0.0, ctx, logprobs, lengths, finished, seen, temp, lpw)
        for a, b in zip(got[:8], want):
            assert torch.equal(a, b)
            if a.dtype == torch.float32:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if with_delta:
        same(BC.LAM, plain(True, BC.LAM))
        same(0.0, plain(False, 0.0))
    else:
        same(0.0, plain(False, 0.0))


def test_prune_lm_argument_errors():
    from nabu_amd import _hip
    key = BC.PRUNE_KEYS[0]
    logits, delta, table, ctx, logprobs, lengths, finished, seen = BC.prune_inputs(key, 0)
    for gamma in (-0.5, float('nan'), float('inf')):
        with pytest.raises(_hip.NabuHipError, match='lm_weight'):
            run_lm(logits, delta, 0.3, table, key[2], gamma, ctx, logprobs, lengths, finished, seen, 1.0, 0.0)
    with pytest.raises(_hip.NabuHipError, match='ctc_weight'):
        run_lm(logits, delta, 1.0, table, key[2], 0.5, ctx, logprobs, lengths, finished, seen, 1.0, 0.0)
    with pytest.raises(_hip.NabuHipError, match='shape'):
        run_lm(logits, delta, 0.3, table, 2, 0.5, ctx, logprobs, lengths, finished, seen, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lam', BC.SEARCH_LAMS, ids=lambda l: 'lam%g' % l)
@pytest.mark.parametrize('kind', BC.SEARCH_KINDS)
def test_lm_beam_search_on_a_tiny_speller(kind, lam, monkeypatch):
    """The SEARCH geometry of beam_joint_cases: W = 40 slots for 13 hypotheses, so the search is exhaustive.  With
    gamma = 0.5 and lambda in {0, 0.3}: every finished hypothesis scores (1 - lambda) log p_att + lambda log p_ctc +
    gamma log p_lm in float64, beams come best first, the best one is the arg-max of the brute-force table.  With an LM
    object and weight 0 the search is the one without, bit for bit, through the entry point it always took."""
    from nabu_amd import _hip
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    from nabu_amd.processing import ngram_lm
    from tests.test_hip_multi_speller import NAMES, make_decoder
    c, seed = J.SEARCH, BC.SEARCH_SEEDS[kind]
    assert BC.search_margin(kind, seed, lam) > BC.MARGIN
    attention, p, encs, enc_lens, ctc_logits = J.search_case(kind, seed)
    table = BC.lm_table(kind, seed)
    lm = ngram_lm.NgramLM(BC.SEARCH_ORDER, c['C'], BC.search_table(seed), ['s%d' % i for i in range(c['C'] - 1)])
    dec = make_decoder(attention, 'softmax', 1, c['U'], J.K_LOC, J.F_LOC, c['C'])
    store = vs.VariableStore(seed=0)
    store.restore_from(device_state(attention, p))
    enc_d = {NAMES[m]: t(e) for m, e in enumerate(encs)}
    lens = {NAMES[m]: SeqLen(l, torch.device(DEV)) for m, l in enumerate(enc_lens)}
    joint = dict(ctc_logits=t(ctc_logits), ctc_weight=lam) if lam else {}
    taken = []
    real_fn = rnn_decoder._Binding.fn
    monkeypatch.setattr(rnn_decoder._Binding, 'fn', lambda self, name: taken.append(name) or real_fn(self, name))
    with torch.no_grad(), vs.as_default(store), vs.variable_scope('Speller'):
        cell = dec.create_cell(enc_d, lens, False)
        args = (cell, list(enc_d.values()), list(lens.values()), c['W'], c['S'], 0.0, 1.0)
        without = rnn_decoder.beam_search(*args, **joint)
        del taken[:]
        zero = rnn_decoder.beam_search(*args, lm=lm, lm_weight=0.0, **joint)
        assert taken[-1] == ('beam_search_joint' if lam else 'beam_search')
        fused = rnn_decoder.beam_search(*args, lm=lm, lm_weight=BC.GAMMA, **joint)
        assert taken[-1] == 'beam_search_ex'
    flat = lambda r: list(r[:3]) + (list(r[3]) if isinstance(r[3], list) else [r[3]])
    for a, b in zip(flat(zero), flat(without)):
        assert torch.equal(a, b)
    assert len(lm._device) == 1                                                  # one upload
    seqs, lengths, scores = (x.cpu().numpy() for x in fused[:3])
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
            want = BC.fused_score(*table[b][g], lam)
            worst = max(worst, abs(got - want) / (1 + abs(want)))
            assert got == pytest.approx(want, rel=SCORE_BOUND, abs=SCORE_BOUND), (b, g)
        assert best == max(table[b], key=lambda g: BC.fused_score(*table[b][g], lam))
    assert np.abs(np.sort(scores, 1) - np.sort(without[2].cpu().numpy(), 1)).max() > 100 * SCORE_BOUND
    print('%s lambda %g: largest score error / (1 + |score|) = %.3g' % (kind, lam, worst))
