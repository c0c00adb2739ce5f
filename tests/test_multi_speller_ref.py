"""CPU tests that pin tests/multi_speller_ref.py, the float64 restatement of the Speller over M encoded inputs, and
the variable names of a two-input Speller.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from tests import multi_speller_ref as MR

CASES = [('vanilla', 'softmax', 1, 0), ('vanilla', 'softmax', 2, 0),
         ('location_aware', 'softmax', 1, 5), ('location_aware', 'softmax', 2, 4),
         ('vanilla', 'sigmoid', 1, 0), ('location_aware', 'normalized_sigmoid', 1, 3),
         ('windowed', 'softmax', 1, 0), ('windowed', 'softmax', 2, 1), ('windowed', 'normalized_sigmoid', 1, 1),
         ('windowed', 'sigmoid', 1, 0)]       # the kinds x probability_fn tests/test_oracle.py parametrises


def _single_params(rng, E, U, C, nl, attention, K=5, F=3):
    p = dict(memory_kernel=rng.normal(0, 0.3, (E, U)), query_kernel=rng.normal(0, 0.3, (U, U)),
             attention_v=rng.normal(0, 0.5, U), out_kernel=rng.normal(0, 0.3, (U + E, C)),
             out_bias=rng.normal(0, 0.1, C), lstm=[])
    for n in range(nl):
        nin = (C + E) if n == 0 else U
        p['lstm'].append(dict(kernel=rng.normal(0, 0.3, (nin + U, 4 * U)), bias=rng.normal(0, 0.1, 4 * U)))
    if attention == 'location_aware':
        p['conv_kernel'] = rng.normal(0, 0.5, (K, F))
        p['conv_proj'] = rng.normal(0, 0.5, (F, U))
    return p


def _targets(rng, B, C, tl):
    t = rng.integers(0, C - 1, (B, int(max(tl))))
    for b in range(B):
        t[b, tl[b] - 1] = C - 1
    return t


@pytest.mark.parametrize('attention,prob_fn,nl,K', CASES)
def test_one_memory_reproduces_the_oracle(attention, prob_fn, nl, K):
    rng = np.random.default_rng(11)
    B, Te, E, U, C = 3, 7, 6, 5, 6
    enc = rng.normal(size=(B, Te, E))
    enc_len, tl = np.array([7, 5, 3]), np.array([5, 3, 4])
    targets = _targets(rng, B, C, tl)
    p = _single_params(rng, E, U, C, nl, attention, K=K)
    window = (K, 2) if attention == 'windowed' else None
    lg, ll, cache = O.speller_fwd(enc, enc_len, targets, tl, p, attention, prob_fn, window=window)
    _, dlg = O.average_cross_entropy(lg, targets, ll, tl)
    denc, g = O.speller_bwd(dlg, cache)
    lg2, _, cache2 = MR.multi_speller_fwd([enc], [enc_len], targets, tl, MR.from_single(p), attention, prob_fn,
                                          window=window)
    np.testing.assert_allclose(lg2, lg, atol=1e-12)
    denc2, g2 = MR.multi_speller_bwd(dlg, cache2)
    np.testing.assert_allclose(denc2[0], denc, atol=1e-12)
    for k in ('out_kernel', 'out_bias'):
        np.testing.assert_allclose(g2[k], g[k], atol=1e-12, err_msg=k)
    for a, b_ in zip(g2['lstm'], g['lstm']):
        np.testing.assert_allclose(a['kernel'], b_['kernel'], atol=1e-12)
        np.testing.assert_allclose(a['bias'], b_['bias'], atol=1e-12)
    for k, v in g2['mem'][0].items():
        np.testing.assert_allclose(v, g[k], atol=1e-12, err_msg=k)


def _two_memory_case(rng, attention, nl):
    B, C, U = 3, 6, 5
    Tes, Es = (7, 4), (6, 3)
    encs = [rng.normal(size=(B, Te, E)) for Te, E in zip(Tes, Es)]
    enc_lens = [np.array([7, 5, 3]), np.array([1, 4, 2])]
    tl = np.array([5, 1, 4])
    targets = _targets(rng, B, C, tl)
    p = MR.make_params(rng, C, U, list(Es), nl, attention, K=3, F=2)
    return encs, enc_lens, targets, tl, p


@pytest.mark.parametrize('attention,prob_fn,nl', [('vanilla', 'softmax', 1), ('location_aware', 'softmax', 2),
                                                   ('location_aware', 'normalized_sigmoid', 1),
                                                   ('windowed', 'softmax', 1), ('vanilla', 'sigmoid', 2)])
def test_two_memories_gradients_against_central_differences(attention, prob_fn, nl):
    """step 1e-6 and bound 1e-8: those of tests/test_oracle.py for the one-memory decoder"""
    rng = np.random.default_rng(31 + nl)
    encs, enc_lens, targets, tl, p = _two_memory_case(rng, attention, nl)
    window = (1, 2) if attention == 'windowed' else None
    run = lambda e, q: MR.multi_speller_fwd(e, enc_lens, targets, tl, q, attention, prob_fn, window=window)
    loss_of = lambda e, q: O.average_cross_entropy(run(e, q)[0], targets, tl, tl)[0]
    lg, ll, cache = run(encs, p)
    _, dlg = O.average_cross_entropy(lg, targets, ll, tl)
    dencs, g = MR.multi_speller_bwd(dlg, cache)
    eps = 1e-6
    for m, idxs in enumerate([[(0, 0, 0), (1, 4, 5), (2, 2, 3)], [(0, 0, 0), (1, 3, 2), (2, 1, 1)]]):
        for idx in idxs:
            a, b_ = [e.copy() for e in encs], [e.copy() for e in encs]
            a[m][idx] += eps; b_[m][idx] -= eps
            np.testing.assert_allclose(dencs[m][idx], (loss_of(a, p) - loss_of(b_, p)) / (2 * eps), atol=1e-8)
    for (name, arr), (_, garr) in zip(MR.flat_items(p), MR.flat_items(g)):
        for flat in rng.integers(0, arr.size, 3):
            idx = np.unravel_index(flat, arr.shape)
            old = arr[idx]
            arr[idx] = old + eps
            up = loss_of(encs, p)
            arr[idx] = old - eps
            dn = loss_of(encs, p)
            arr[idx] = old
            np.testing.assert_allclose(garr[idx], (up - dn) / (2 * eps), atol=1e-8, err_msg='%s %s' % (name, idx))


@pytest.mark.parametrize('attention,prob_fn,nl', [('vanilla', 'softmax', 2), ('location_aware', 'softmax', 1),
                                                   ('location_aware', 'sigmoid', 2), ('windowed', 'softmax', 1),
                                                   ('windowed', 'normalized_sigmoid', 2)])
def test_two_memories_against_torch_autograd(attention, prob_fn, nl):
    rng = np.random.default_rng(47)
    encs, enc_lens, targets, tl, p = _two_memory_case(rng, attention, nl)
    window = (1, 2) if attention == 'windowed' else None
    lg, ll, cache = MR.multi_speller_fwd(encs, enc_lens, targets, tl, p, attention, prob_fn, window=window)
    w = rng.normal(size=lg.shape)                       # a generic linear functional of the logits
    dencs, g = MR.multi_speller_bwd(w, cache)
    lgt, leaves = MR.torch_multi_speller(encs, enc_lens, targets, tl, p, attention, prob_fn, window)
    np.testing.assert_allclose(lg, lgt.detach().numpy(), atol=1e-11)
    (lgt * torch.tensor(w)).sum().backward()
    for m in range(2):
        mask = (np.arange(encs[m].shape[1])[None, :] < enc_lens[m][:, None])[:, :, None]
        np.testing.assert_allclose(dencs[m], leaves['enc'][m].grad.numpy() * mask, atol=1e-11)
    for name, garr in MR.flat_items(g):
        np.testing.assert_allclose(garr, leaves[name].grad.numpy(), atol=1e-11, err_msg=name)


def _cell_names(n_inputs, attention):
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder, speller
    conf = dict(dropout='1', num_units='8', num_layers='2', attention=attention, probability_fn='softmax',
                numfilt='2', filtersize='3', left_window_width='1', right_window_width='2')
    dec = speller.Speller.__new__(speller.Speller)
    dec.conf, dec.output_dims = conf, {'text': 5}
    names = ['features', 'aux'][:n_inputs]
    encoded = {n: torch.zeros(2, 6 + 3 * i, 4 + 4 * i) for i, n in enumerate(names)}
    lens = {n: np.array([6, 3]) for n in names}
    store = vs.VariableStore(seed=0, device=torch.device('cpu'))
    with vs.as_default(store), vs.variable_scope('Speller'):
        cell = dec.create_cell(encoded, lens, False)
        Es = [int(encoded[n].shape[2]) for n in names]
        rnn_decoder.cell_parameters(cell, Es if n_inputs > 1 else Es[0])
    return store


@pytest.mark.parametrize('attention,scope', [('location_aware', 'location_aware_attention'),
                                             ('vanilla', 'bahdanau_attention'), ('windowed', 'windowed_attention')])
def test_variable_names_of_a_two_input_speller(attention, scope):
    """mechanism 0 keeps the one-input names; mechanism 1 gets TF's uniquified scopes"""
    one, two = _cell_names(1, attention), _cell_names(2, attention)
    pre = 'Speller/decoder/'
    mech = ['memory_layer%s/kernel', scope + '%s/query_layer/kernel', scope + '%s/attention_v']
    if attention == 'location_aware':
        mech += [scope + '%s/conv1d/kernel', scope + '%s/process_conv_features/kernel']
    shared = ['attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/%s' % (n, k) for n in range(2) for k in ('kernel', 'bias')]
    shared += ['dense/kernel', 'dense/bias']
    assert set(one.order) == {pre + n % '' for n in mech} | {pre + n for n in shared}
    assert set(two.order) == {pre + n % s for n in mech for s in ('', '_1')} | {pre + n for n in shared}
    assert set(two.state_dict().keys()) == set(two.order)          # the TF-named export lists them
    # memory 1 is [.., .., 8] wide, memory 0 [.., .., 4]: its own memory layer; layer 0 and the projection take both
    assert two.vars[pre + 'memory_layer_1/kernel'].shape == (8, 8) and two.vars[pre + 'memory_layer/kernel'].shape == (4, 8)
    assert two.vars[pre + 'attention_wrapper/multi_rnn_cell/cell_0/lstm_cell/kernel'].shape == (5 + 12 + 8, 32)
    assert two.vars[pre + 'dense/kernel'].shape == (8 + 12, 5)
