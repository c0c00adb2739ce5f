"""GPU parity of the Speller over several encoded inputs (one attention mechanism each; nabu_speller_multi_*,
speller_multi.hip) against the float64 restatement tests/multi_speller_ref.py, through the decoder of the recipe API.

Bounds: those tests/test_hip_speller.py applies to the one-memory step chain for the same quantities — 2e-5 absolute on
the logits, 2e-4 relative (to the largest entry) on every gradient: it is the same arithmetic per mechanism.

Attention geometry: a mechanism's workgroups cut an utterance into S = nabu_attn_bwd_slices frame slices.  The small
shapes (<= 16 frames) run with S = 1, the larger case (B = 32, Te = (40, 64)) with S = (3, 4) — a different slice count
per mechanism inside one launch; the tests assert both through nabu_speller_multi_attn_slices."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from nabu_amd import recipes
from tests import multi_speller_ref as MR

pytestmark = pytest.mark.gpu

PRE = 'Speller/decoder/'
SCOPES = {'vanilla': 'bahdanau_attention', 'location_aware': 'location_aware_attention', 'windowed': 'windowed_attention'}
NAMES = ['features', 'aux', 'third']


def mech_names(attention, m):
    sc, sx = SCOPES[attention], ('_%d' % m if m else '')
    n = dict(memory_kernel=PRE + 'memory_layer%s/kernel' % sx, query_kernel=PRE + sc + sx + '/query_layer/kernel',
             attention_v=PRE + sc + sx + '/attention_v')
    if attention == 'location_aware':
        n.update(conv_kernel=PRE + sc + sx + '/conv1d/kernel', conv_proj=PRE + sc + sx + '/process_conv_features/kernel')
    return n


def ref_params(st, nl, attention, M):
    f = lambda a: a.astype(np.float64)
    p = dict(out_kernel=f(st[PRE + 'dense/kernel']), out_bias=f(st[PRE + 'dense/bias']), lstm=[], mem=[])
    for n in range(nl):
        q = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        p['lstm'].append(dict(kernel=f(st[q + 'kernel']), bias=f(st[q + 'bias'])))
    for m in range(M):
        pm = {k: f(st[name]) for k, name in mech_names(attention, m).items()}
        if 'conv_kernel' in pm:
            pm['conv_kernel'] = pm['conv_kernel'].reshape(pm['conv_kernel'].shape[0], -1)
        p['mem'].append(pm)
    return p


def make_decoder(attention, prob_fn, nl, U, K, F, C, extra=None):
    from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory
    over = {'decoder.num_layers': nl, 'decoder.num_units': U, 'decoder.attention': attention,
            'decoder.probability_fn': prob_fn}
    if attention == 'location_aware':
        over.update({'decoder.numfilt': F, 'decoder.filtersize': K})
    if attention == 'windowed':
        over.update({'decoder.left_window_width': K, 'decoder.right_window_width': F})
    over.update(extra or {})
    mc, _, _ = recipes.load_recipe('cfg3_las_vanilla', **over)
    return ed_decoder_factory.factory('speller')(mc, {'text': C}, None)


def make_data(seed, B, Tes, Es, enc_lens, tlen, C):
    rng = np.random.default_rng(seed)
    encs = []
    for Te, E, el in zip(Tes, Es, enc_lens):
        e = rng.normal(size=(B, Te, E)).astype(np.float32)
        encs.append(e * (np.arange(Te)[None, :, None] < np.asarray(el)[:, None, None]))
    Lmax = int(max(tlen)) + 1
    tg = rng.integers(0, C - 1, (B, Lmax)).astype(np.int32)
    for b in range(B):
        tg[b, tlen[b] - 1] = C - 1
        tg[b, tlen[b]:] = 0
    return encs, tg


def run_device(dec, encs, enc_lens, tg, tlen, store=None, seed=3, training=True):
    """forward + loss + backward on the device; returns (logits, loss, [d enc_m], store)"""
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import Tape, SeqLen, record
    from nabu_amd.neuralnetworks.trainers import loss_functions
    dev = torch.device('cuda')
    M = len(encs)
    store = store or vs.VariableStore(seed=seed)
    for v in store.vars.values():
        v.grad = None
    src = [torch.tensor(e, device=dev) for e in encs]
    enc_d = [torch.tensor(e, device=dev) for e in encs]
    tgd = {'text': torch.tensor(tg, device=dev)}
    with vs.as_default(store), Tape() as tape:
        for s, e in zip(src, enc_d):
            record([s], [e], lambda g: [g])
        logits, lsl, _ = dec({NAMES[m]: enc_d[m] for m in range(M)},
                             {NAMES[m]: SeqLen(np.asarray(enc_lens[m], np.int32), dev) for m in range(M)},
                             tgd, {'text': SeqLen(tlen, dev)}, training)
        loss = loss_functions.average_cross_entropy(tgd, logits, lsl, {'text': SeqLen(tlen, dev)})
    got = [None] * M
    for m in range(M):
        def capture(g, m=m):
            got[m] = g
            return [None]
        tape.ops[m].backward = capture
    tape.backward(loss)
    torch.cuda.synchronize()
    return logits['text'].cpu().numpy(), float(loss.item()), [g.cpu().numpy() for g in got], store


def slices_of(B, U, C, L, nl, Tes, Es, kind=0, K=0, F=0):
    from nabu_amd import _hip
    M = len(Tes)
    i4 = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES
    d = _hip.SpellerMultiDesc(ctypes.sizeof(_hip.SpellerMultiDesc), M, B, U, C, L, nl, i4(*(list(Tes) + [0] * (4 - M))),
                              i4(*(list(Es) + [0] * (4 - M))), kind, K, F, 0, 1.0, 0, 0, 0.0, 0, 0)
    lib = _hip.lib()
    assert lib.nabu_speller_multi_uses_persistent(ctypes.byref(d), 0) == 0
    assert lib.nabu_speller_multi_uses_persistent(ctypes.byref(d), 1) == 0
    return [lib.nabu_speller_multi_attn_slices(ctypes.byref(d), m) for m in range(M)]


def check_multi(attention, prob_fn, nl, U, K, F, Tes, Es, enc_lens, tlen, C=6, seed=5):
    B, M = len(tlen), len(Tes)
    tlen = np.asarray(tlen, np.int32)
    dec = make_decoder(attention, prob_fn, nl, U, K, F, C)
    encs, tg = make_data(seed, B, Tes, Es, enc_lens, tlen, C)
    lg, loss, dencs, store = run_device(dec, encs, enc_lens, tg, tlen)
    p = ref_params(store.state_dict(), nl, attention, M)
    rl, rll, cache = MR.multi_speller_fwd([e.astype(np.float64) for e in encs], enc_lens, tg, tlen, p, attention,
                                          prob_fn, window=(K, F) if attention == 'windowed' else None)
    err = np.abs(lg - rl).max()
    print('logits abs err %.3g' % err)
    assert err < 2e-5
    for b in range(B):
        assert np.all(lg[b, tlen[b]:] == 0)
    rloss, dlg = O.average_cross_entropy(rl, tg, rll, tlen)
    assert abs(loss - rloss) / rloss < 1e-5
    rdencs, rg = MR.multi_speller_bwd(dlg, cache)
    rel = lambda a, b_: np.abs(a - b_).max() / (np.abs(b_).max() + 1e-12)
    for m in range(M):
        e = rel(dencs[m], rdencs[m])
        print('d enc[%d] rel err %.3g' % (m, e))
        assert e < 2e-4, m
        for k, name in mech_names(attention, m).items():
            g = store.vars[name].grad.cpu().numpy().astype(np.float64).reshape(rg['mem'][m][k].shape)
            e = rel(g, rg['mem'][m][k])
            print('%s rel err %.3g' % (name, e))
            assert e < 2e-4, (m, k)
    for k in ('out_kernel', 'out_bias'):
        assert rel(store.vars[PRE + 'dense/' + k[4:]].grad.cpu().numpy(), rg[k]) < 2e-4, k
    for n in range(nl):
        q = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        assert rel(store.vars[q + 'kernel'].grad.cpu().numpy(), rg['lstm'][n]['kernel']) < 2e-4, n
        assert rel(store.vars[q + 'bias'].grad.cpu().numpy(), rg['lstm'][n]['bias']) < 2e-4, n
    return lg


SMALL = dict(Tes=(7, 12), Es=(8, 24), enc_lens=[np.array([7, 1, 4]), np.array([12, 5, 1])], tlen=[5, 1, 3])


@pytest.mark.parametrize('prob_fn', ['softmax', 'normalized_sigmoid'])
@pytest.mark.parametrize('attention,K,F', [('vanilla', 0, 0), ('location_aware', 3, 2), ('windowed', 1, 2)])
@pytest.mark.parametrize('nl', [1, 2])
def test_two_memories_match_the_float64_restatement(nl, attention, K, F, prob_fn):
    """unequal Te and E: a wrong column offset into the [B, sum E] rows, a wrong row stride or a workgroup using the
    other memory's Te shows here; an encoder length of 1 in each memory, a row finished after step 1"""
    assert slices_of(3, 16, 6, 5, nl, SMALL['Tes'], SMALL['Es']) == [1, 1]
    check_multi(attention, prob_fn, nl, 16, K, F, **SMALL)


@pytest.mark.parametrize('attention,K,F', [('vanilla', 0, 0), ('location_aware', 3, 2)])
def test_wide_decoder(attention, K, F):
    """U = 512: lanes own two 16-byte unit groups (the j > 0 iterations of both kernels' unit loops) and the cross-wave
    reductions run at their realistic width; Te = (20, 33) at B = 3 gives 2 and 3 frame slices"""
    assert slices_of(3, 512, 6, 4, 1, (20, 33), (8, 24)) == [2, 3]
    check_multi(attention, 'softmax', 1, 512, K, F, Tes=(20, 33), Es=(8, 24),
                enc_lens=[np.array([20, 1, 11]), np.array([33, 17, 2])], tlen=[4, 1, 3])


@pytest.mark.parametrize('attention,K,F', [('vanilla', 0, 0), ('location_aware', 3, 2)])
def test_three_memories(attention, K, F):
    check_multi(attention, 'softmax', 1, 16, K, F, Tes=(5, 5, 9), Es=(8, 4, 12),
                enc_lens=[np.array([5, 2, 1]), np.array([3, 5, 5]), np.array([9, 1, 6])], tlen=[4, 5, 1])


@pytest.mark.parametrize('attention,prob_fn,K,F', [('vanilla', 'softmax', 0, 0), ('location_aware', 'softmax', 5, 3),
                                                    ('windowed', 'normalized_sigmoid', 2, 3), ('vanilla', 'sigmoid', 0, 0)])
def test_frame_sliced_geometry_with_a_slice_count_per_memory(attention, prob_fn, K, F):
    """B = 32, Te = (40, 64): 3 and 4 frame slices per utterance in ONE launch (the last slice to arrive finishes its
    utterance: softmax rescaling forward; dq, d previous alignment and d conv kernel backward)"""
    rng = np.random.default_rng(9)
    B = 32
    assert slices_of(B, 32, 6, 6, 1, (40, 64), (64, 32)) == [3, 4]
    el = [rng.integers(1, 41, B), rng.integers(20, 65, B)]
    el[0][0], el[1][0], el[1][5] = 40, 64, 1
    tlen = rng.integers(1, 7, B)
    tlen[2] = 6
    check_multi(attention, prob_fn, 1, 32, K, F, Tes=(40, 64), Es=(64, 32), enc_lens=el, tlen=tlen)


@pytest.mark.parametrize('attention,K,F', [('vanilla', 0, 0), ('location_aware', 3, 2), ('windowed', 1, 2)])
def test_one_memory_through_the_new_entry_points_equals_the_existing_ones(attention, K, F, monkeypatch):
    """guards the generalisation itself: the same decoder, M = 1, once through nabu_speller_* and once through
    nabu_speller_multi_*"""
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    tlen = np.asarray(SMALL['tlen'], np.int32)
    dec = make_decoder(attention, 'softmax', 2, 16, K, F, 6)
    encs, tg = make_data(5, 3, SMALL['Tes'][:1], SMALL['Es'][:1], SMALL['enc_lens'][:1], tlen, 6)
    lg0, loss0, d0, store = run_device(dec, encs, SMALL['enc_lens'][:1], tg, tlen)
    assert not hasattr(rnn_decoder.dynamic_decode.last[0], 'M')          # the one-memory descriptor
    g0 = {n: v.grad.cpu().numpy().copy() for n, v in store.vars.items()}
    monkeypatch.setattr(rnn_decoder, '_force_multi', True)
    lg1, loss1, d1, _ = run_device(dec, encs, SMALL['enc_lens'][:1], tg, tlen, store=store)
    assert rnn_decoder.dynamic_decode.last[0].M == 1
    assert np.abs(lg1 - lg0).max() < 2e-5
    rel = lambda a, b_: np.abs(a - b_).max() / (np.abs(b_).max() + 1e-12)
    assert rel(d1[0], d0[0]) < 2e-4
    for n, v in store.vars.items():
        assert rel(v.grad.cpu().numpy(), g0[n]) < 2e-4, n


@pytest.mark.parametrize('attention,K,F', [('location_aware', 3, 2), ('vanilla', 0, 0)])
def test_identical_calls_give_identical_bits(attention, K, F):
    rng = np.random.default_rng(9)
    B = 32
    el = [rng.integers(1, 41, B), rng.integers(20, 65, B)]
    tlen = rng.integers(1, 7, B).astype(np.int32)
    dec = make_decoder(attention, 'softmax', 2, 32, K, F, 6)
    encs, tg = make_data(6, B, (40, 64), (64, 32), el, tlen, 6)
    lg0, loss0, d0, store = run_device(dec, encs, el, tg, tlen)
    g0 = {n: v.grad.cpu().numpy().copy() for n, v in store.vars.items()}
    lg1, loss1, d1, _ = run_device(dec, encs, el, tg, tlen, store=store)
    np.testing.assert_array_equal(lg0, lg1)
    for a, b_ in zip(d0, d1):
        np.testing.assert_array_equal(a, b_)
    for n, v in store.vars.items():
        np.testing.assert_array_equal(v.grad.cpu().numpy(), g0[n], err_msg=n)


@pytest.mark.parametrize('nl,dropout,C', [(1, 1.0, 6), (2, 0.5, 6), (1, 1.0, 8), (2, 0.5, 8)])
def test_sampling_and_dropout_draws_do_not_depend_on_the_number_of_memories(nl, dropout, C):
    """memory 2 with zero values and a zero block in the projection: its context is zero, the logits are those of the
    one-memory decoder, so under the same seeds the sampled decoder inputs must be the same (scheduled sampling draws
    counter (row, offset + step); the dropout masks (step, layer))"""
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    # C = 8: the one-launch sampling step (C % 4 == 0, C <= 256); C = 6: the step's projection as two products
    # ([h | contexts] against out_kernel's rows 0..U and U..U + sum E) + the sampling kernel
    B, U = 8, 16
    Tes, Es = (7, 12), (8, 24)
    rng = np.random.default_rng(12)
    el = [rng.integers(1, 8, B), rng.integers(1, 13, B)]
    tlen = rng.integers(2, 7, B).astype(np.int32)
    tlen[0] = 6
    dec = make_decoder('vanilla', 'softmax', nl, U, 0, 0, C, {'decoder.sample_prob': 0.5, 'decoder.dropout': dropout})
    encs, tg = make_data(8, B, Tes, Es, el, tlen, C)
    nops.set_seed(77)
    lg1, _, _, store1 = run_device(dec, encs[:1], el[:1], tg, tlen)
    used1 = rnn_decoder.decoder_inputs().cpu().numpy().copy()
    teacher = np.concatenate([np.full((1, B), C - 1), tg[:, :int(tlen.max()) - 1].T], 0)
    assert (used1 != teacher).any()                       # something was sampled
    # the two-memory decoder with the one-memory decoder's parameters; zero rows for memory 2 in the projection
    st = store1.state_dict()
    k0 = PRE + 'attention_wrapper/multi_rnn_cell/cell_0/lstm_cell/kernel'
    restore = dict(st)
    restore[k0] = np.concatenate([st[k0][:C + Es[0]], rng.normal(0, 0.3, (Es[1], 4 * U)).astype(np.float32),
                                  st[k0][C + Es[0]:]], 0)
    restore[PRE + 'dense/kernel'] = np.concatenate([st[PRE + 'dense/kernel'], np.zeros((Es[1], C), np.float32)], 0)
    store2 = vs.VariableStore(seed=4)
    store2.restore = restore
    encs2 = [encs[0], np.zeros_like(encs[1])]
    nops.set_seed(77)
    lg2, _, _, _ = run_device(dec, encs2, el, tg, tlen, store=store2)
    used2 = rnn_decoder.decoder_inputs().cpu().numpy()
    np.testing.assert_array_equal(used2, used1)
    assert np.abs(lg2 - lg1).max() < 2e-5


BEAM = dict(B=2, W=3, Tes=(6, 9), Es=(8, 12), U=16, C=5, S=4, enc_lens=[np.array([6, 3]), np.array([4, 9])], seed=1)
BEAM_BOUND = 2e-4         # rtol = atol of the scores in tests/test_hip_decode.py


def beam_cell(c, attention, K, F, nl=1):
    """decoder and encoded arrays of a BEAM-shaped case"""
    dec = make_decoder(attention, 'softmax', nl, c['U'], K, F, c['C'])
    encs, _ = make_data(c['seed'], c['B'], c['Tes'], c['Es'], c['enc_lens'], np.array([1, 1]), c['C'])
    return dec, encs


@pytest.mark.parametrize('attention,K,F,seed', [('vanilla', 0, 0, 2), ('location_aware', 3, 2, 5)])
def test_beam_search_over_two_memories_against_brute_force(attention, K, F, seed):
    """M = 2, B = 2, W = 3, Te = (6, 9): sequences, lengths, scores and the alignments of BOTH memories against the
    float64 enumeration of tests/multi_speller_ref.py, which carries no state (every hypothesis is re-evaluated from
    its prefix).  The reference's neighbouring candidate scores must be more than 100 x the score bound apart, checked
    here on the CPU: a near-tie could hide a wrong path."""
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    c = dict(BEAM, seed=seed)          # (seeds chosen on the CPU for the reference's separation, asserted below)
    dev = torch.device('cuda')
    dec, encs = beam_cell(c, attention, K, F)
    store = vs.VariableStore(seed=c['seed'])
    enc_d = {NAMES[m]: torch.tensor(encs[m], device=dev) for m in range(2)}
    lens = {NAMES[m]: SeqLen(c['enc_lens'][m].astype(np.int32), dev) for m in range(2)}
    with torch.no_grad(), vs.as_default(store), vs.variable_scope('Speller'):
        cell = dec.create_cell(enc_d, lens, False)
        seqs, lengths, scores, aligns = rnn_decoder.beam_search(cell, list(enc_d.values()), list(lens.values()), c['W'], c['S'],
                                                                0.0, 1.0)
    p = ref_params(store.state_dict(), 1, attention, 2)
    ref, gap, steps = MR.brute_force_beam_search([e.astype(np.float64) for e in encs], c['enc_lens'], p, c['W'], c['S'],
                                                 attention)
    print('smallest gap between neighbouring candidates %.4f, steps %d' % (gap, steps))
    assert gap > 100 * BEAM_BOUND, gap
    seqs, lengths, scores = seqs.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()
    assert seqs.shape == (c['B'], c['W'], steps) and isinstance(aligns, list) and len(aligns) == 2
    for m in range(2):
        assert tuple(aligns[m].shape) == (c['B'], c['W'], steps, c['Tes'][m])
    for b in range(c['B']):
        for w in range(c['W']):
            lab, ln, lp, fin, _, als = ref[b][w]
            np.testing.assert_array_equal(seqs[b, w, :len(lab)], np.array(lab))
            np.testing.assert_array_equal(lengths[b, w], ln)
            np.testing.assert_allclose(scores[b, w], lp, rtol=BEAM_BOUND, atol=BEAM_BOUND)
            for m in range(2):
                a = aligns[m][b, w].cpu().numpy()
                for t in range(len(als[m])):
                    np.testing.assert_allclose(a[t], als[m][t], atol=2e-5)


# the BEAM case restricted to its first memory, and 40 frames with lengths (40, 20): more than the 32 frames of a slice,
# so both attention implementations run frame-sliced (tests/test_hip_decode.py uses 40 frames for the same purpose)
ONE_BEAM = dict(BEAM, Tes=BEAM['Tes'][:1], Es=BEAM['Es'][:1], enc_lens=BEAM['enc_lens'][:1])
ONE_BEAM_40 = dict(ONE_BEAM, Tes=(40,), enc_lens=[np.array([40, 20])])


@pytest.mark.parametrize('attention,K,F,case,seed,sliced', [('vanilla', 0, 0, ONE_BEAM, 40, False),
                                                            ('location_aware', 3, 2, ONE_BEAM, 36, False),
                                                            ('location_aware', 3, 2, ONE_BEAM_40, 49, True)])
def test_one_memory_through_both_beam_search_entry_points(attention, K, F, case, seed, sliced, monkeypatch):
    """guards the shared beam-search loop: the same decoder and the same single memory once through
    nabu_speller_beam_search (nabu_attn_fwd) and once through nabu_speller_multi_beam_search with M = 1
    (multi_attn_fwd).  The two attention kernels round differently, so a near-tie between candidates could order
    differently: the float64 enumeration must keep neighbouring candidate scores more than 100 x the score bound apart
    (seeds chosen on the CPU for that, asserted below)."""
    from nabu_amd import _hip, variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    c = dict(case, seed=seed)
    dev = torch.device('cuda')
    # the geometry of the B * W rows in both implementations: one workgroup per row, or frame slices with partials
    N, kind = c['B'] * c['W'], {'vanilla': 0, 'location_aware': 1}[attention]
    ad = _hip.AttnDesc(ctypes.sizeof(_hip.AttnDesc), N, c['Tes'][0], c['Es'][0], c['U'], kind, K, F, 0)
    assert (_hip.lib().nabu_attn_fwd_ws_bytes(ctypes.byref(ad)) > 0) == sliced
    assert (slices_of(N, c['U'], c['C'], 1, 1, c['Tes'], c['Es'], kind, K, F)[0] > 1) == sliced
    dec, encs = beam_cell(c, attention, K, F)
    store = vs.VariableStore(seed=c['seed'])
    enc_d = {'features': torch.tensor(encs[0], device=dev)}
    lens = {'features': SeqLen(c['enc_lens'][0].astype(np.int32), dev)}
    with torch.no_grad(), vs.as_default(store), vs.variable_scope('Speller'):
        cell = dec.create_cell(enc_d, lens, False)
        args = (cell, list(enc_d.values()), list(lens.values()), c['W'], c['S'], 0.0, 1.0)
        seqs0, lengths0, scores0, aligns0 = rnn_decoder.beam_search(*args)
        monkeypatch.setattr(rnn_decoder, '_force_multi', True)
        seqs1, lengths1, scores1, aligns1 = rnn_decoder.beam_search(*args)
    # the one-memory entry point returns the alignments as a tensor, the multi one as a list per memory
    assert torch.is_tensor(aligns0) and isinstance(aligns1, list) and len(aligns1) == 1
    p = ref_params(store.state_dict(), 1, attention, 1)
    _, gap, steps = MR.brute_force_beam_search([encs[0].astype(np.float64)], c['enc_lens'], p, c['W'], c['S'], attention)
    print('smallest gap between neighbouring candidates %.4f, steps %d' % (gap, steps))
    assert gap > 100 * BEAM_BOUND, gap
    assert seqs0.shape == seqs1.shape == (c['B'], c['W'], steps)
    np.testing.assert_array_equal(seqs1.cpu().numpy(), seqs0.cpu().numpy())
    np.testing.assert_array_equal(lengths1.cpu().numpy(), lengths0.cpu().numpy())
    err = np.abs(scores1.cpu().numpy() - scores0.cpu().numpy()).max()
    aerr = np.abs(aligns1[0].cpu().numpy() - aligns0.cpu().numpy()).max()
    print('scores abs diff %.3g, alignments abs diff %.3g' % (err, aerr))
    np.testing.assert_allclose(scores1.cpu().numpy(), scores0.cpu().numpy(), rtol=BEAM_BOUND, atol=BEAM_BOUND)
    assert tuple(aligns0.shape) == tuple(aligns1[0].shape) == (c['B'], c['W'], steps, c['Tes'][0])
    np.testing.assert_allclose(aligns1[0].cpu().numpy(), aligns0.cpu().numpy(), atol=2e-5)


def test_beam_search_decoder_gives_alignments_per_input_name():
    """through decoders/beam_search_decoder.py: a two-input model decodes, the alignments come as a dict per input"""
    from nabu_amd.neuralnetworks.decoders import beam_search_decoder
    tr, data = two_input_trainer()
    b = tr.to_device(data.batch(0))
    tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)
    alphabet = ' '.join('s%d' % i for i in range(list(tr.model.output_dims.values())[0]))
    import configparser
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': {'decoder': 'beam_search_decoder', 'alphabet': alphabet, 'max_steps': '4', 'beam_width': '3',
                                'length_penalty': '0.0', 'temperature': '1.0', 'visualize_alignments': 'True'}})
    dec = beam_search_decoder.BeamSearchDecoder(conf, tr.model)
    seqs, lengths, scores, aligns = dec(b['inputs'], b['input_seq_length'])['text']
    assert set(aligns.keys()) == {'features', 'aux'}
    assert aligns['features'].shape[:2] == aligns['aux'].shape[:2] == seqs.shape[:2]
    assert aligns['features'].shape[3] != aligns['aux'].shape[3]
    assert torch.isfinite(scores).all()


class TwoStreams(object):
    """two synthetic feature streams of different dimension and length under the names 'features' and 'aux'"""

    def __init__(self, B, a=None, b=None):
        from nabu_amd.processing.synthetic import SyntheticData
        self.a = a or SyntheticData(B, 64, 40, min_frames=40, min_labels=2, max_labels=6, eos=True, time_reduction=8,
                                    seed=3234)
        self.b = b or SyntheticData(B, 40, 12, min_frames=17, min_labels=2, max_labels=6, eos=True, time_reduction=8,
                                    seed=77, input_name='aux')

    def num_batches(self):
        return self.a.num_batches()

    def validation(self, numbatches, batch_size=None):
        return TwoStreams(batch_size, self.a.validation(numbatches, batch_size), self.b.validation(numbatches, batch_size))

    def batch(self, step):
        x, y = self.a.batch(step), self.b.batch(step)
        x['inputs']['aux'] = y['inputs']['aux']
        x['input_seq_length']['aux'] = y['input_seq_length']['aux']
        return x


def two_input_trainer(B=4):
    from tests.test_hip_model import make_trainer
    data = TwoStreams(B)
    over = {'io.inputs': 'features aux', 'encoder.num_units': 32, 'decoder.num_units': 32, 'trainer.batch_size': B,
            'encoder.gemm_precision': 'f32'}
    return make_trainer('cfg3_las_vanilla', data, **over), data


def test_two_input_las_training_trajectory_matches_the_float64_restatement():
    """shrunken cfg3 with inputs = features aux (a listener on each, two attention mechanisms): 10 clip+Adam steps
    against the oracle's listener and tests/multi_speller_ref.py; the largest relative loss error must be <= 1e-3
    (the project's parity bar, README.md).  Fails on a tree without the feature with the Speller's
    NotImplementedError.  Measured: see this test's print and LABNOTES.md section 13."""
    from tests.test_hip_model import encoder_layers
    STEPS = 10
    tr, data = two_input_trainer()
    losses = [float(tr.step(tr.to_device(data.batch(s))).item()) for s in range(STEPS)]
    tr2, _ = two_input_trainer()
    b0 = tr2.to_device(data.batch(0))
    tr2.model(b0['inputs'], b0['input_seq_length'], b0['targets'], b0['target_seq_length'], False)
    st = tr2.model.store.state_dict()
    assert 'Speller/decoder/memory_layer_1/kernel' in st and 'Speller/decoder/bahdanau_attention_1/attention_v' in st
    names = ['features', 'aux']
    lay = {n: encoder_layers({k.replace('Listener/%s/' % n, 'Listener/features/'): v for k, v in st.items()
                              if k.startswith('Listener/%s/' % n)}, 'Listener', 3) for n in names}
    p = ref_params(st, 1, 'vanilla', 2)

    def leaves():
        v = []
        for n in names:
            for l in lay[n]:
                v += [(l, k) for k in ('fw_kernel', 'fw_bias', 'bw_kernel', 'bw_bias')]
        v += [(p, 'out_kernel'), (p, 'out_bias'), (p['lstm'][0], 'kernel'), (p['lstm'][0], 'bias')]
        for pm in p['mem']:
            v += [(pm, k) for k in sorted(pm)]
        return v
    lv = leaves()
    ms = [np.zeros_like(h[k]) for h, k in lv]
    vs_ = [np.zeros_like(h[k]) for h, k in lv]
    ref = []
    for s in range(STEPS):
        b = data.batch(s)
        encs, els, caches = [], [], []
        for n in names:
            e, el, ca = O.listener_fwd(b['inputs'][n].astype(np.float64), b['input_seq_length'][n], lay[n])
            encs.append(e); els.append(el); caches.append(ca)
        tg, tl = b['targets']['text'], b['target_seq_length']['text']
        lg, ll, cache = MR.multi_speller_fwd(encs, els, tg, tl, p)
        loss, dlg = O.average_cross_entropy(lg, tg, ll, tl)
        ref.append(loss)
        dencs, g = MR.multi_speller_bwd(dlg, cache)
        grads = []
        for i, n in enumerate(names):
            _, gl = O.listener_bwd(dencs[i], caches[i])
            for l in gl:
                grads += [l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias']]
        grads += [g['out_kernel'], g['out_bias'], g['lstm'][0]['kernel'], g['lstm'][0]['bias']]
        for gm in g['mem']:
            grads += [gm[k] for k in sorted(gm)]
        for i, ((h, k), gr) in enumerate(zip(lv, grads)):
            h[k], ms[i], vs_[i] = O.clip_adam_update(h[k], gr, ms[i], vs_[i], s + 1, 1e-3)
    rel = np.abs(np.array(losses) - np.array(ref)) / np.abs(ref)
    print('two-input LAS, %d steps: largest relative loss error %.3g' % (STEPS, rel.max()))
    assert rel.max() <= 1e-3, (losses, ref)
