"""CPU: the keys of joint CTC/attention training and decoding — ctc_head in the model's [decoder] section, ctc_weight in
[trainer] and in the beam search decoder's conf.  Their validation, what refuses them, and that a configuration without
them creates the variables and makes the calls it always did."""
import configparser
import os
import re

import pytest
import torch

from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = {'decoder.ctc_head': 'True'}


def _trainer(recipe='cfg3_las_vanilla', **over):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(4, 32, 40), modelconf=mc,
                                               evaluatorconf=ec, expdir=None, server=None, task_index=0)


# ------------------------------------------------------------------------------------------------------- the keys
@pytest.mark.parametrize('value', ['abc', '-0.1', '1', '1.5', 'nan'])
def test_trainer_refuses_a_bad_weight_naming_the_key(value):
    with pytest.raises(ValueError, match='ctc_weight'):
        _trainer(**dict(HEAD, **{'trainer.ctc_weight': value}))


def test_weight_with_the_ctc_loss_is_refused_at_construction():
    with pytest.raises(ValueError, match='loss = CTC is that term alone'):
        _trainer('cfg2_listener_ctc', **{'trainer.ctc_weight': 0.3})
    assert _trainer('cfg2_listener_ctc', **{'trainer.ctc_weight': 0}).ctc_weight == 0.0


def test_weight_without_a_head_is_refused_and_a_head_without_weight_is_not():
    with pytest.raises(ValueError, match='ctc_head = True'):
        _trainer(**{'trainer.ctc_weight': 0.3})
    tr = _trainer(**HEAD)
    assert tr.ctc_weight == 0.0 and tr.model.decoder.ctc_head
    tr = _trainer(**dict(HEAD, **{'trainer.ctc_weight': 0}))
    assert tr.ctc_weight == 0.0
    tr = _trainer(**dict(HEAD, **{'trainer.ctc_weight': 0.3, 'trainer.label_smoothing': 0.1}))
    assert (tr.ctc_weight, tr.label_smoothing) == (0.3, 0.1)
    plain = _trainer()
    assert 'ctc_weight' not in plain.conf and plain.ctc_weight == 0.0 and not plain.model.decoder.ctc_head


@pytest.mark.parametrize('value', ['yes', '1', 'true', ''])
def test_a_head_key_that_is_neither_true_nor_false_is_refused(value):
    with pytest.raises(ValueError, match='ctc_head'):
        _trainer(**{'decoder.ctc_head': value})
    assert not _trainer(**{'decoder.ctc_head': 'False'}).model.decoder.ctc_head


@pytest.mark.parametrize('recipe', ['cfg2_listener_ctc', 'dnn_hybrid_wsj'])
def test_a_head_on_a_dnn_decoder_is_refused_at_construction(recipe):
    with pytest.raises(ValueError, match='recurrent attention decoder'):
        _trainer(recipe, **HEAD)


def test_factory_binds_the_weight_into_the_cross_entropy_losses_only():
    from nabu_amd.neuralnetworks.trainers import loss_functions as lf
    assert lf.factory('average_cross_entropy', 0.0, 0.0) is lf.average_cross_entropy
    assert lf.factory('sum_cross_entropy', ctc_weight=0) is lf.sum_cross_entropy
    for name in ('average_cross_entropy', 'sum_cross_entropy'):
        fn = lf.factory(name, ctc_weight=0.3)
        assert fn.func is getattr(lf, name) and fn.keywords == {'ctc_weight': 0.3}
        fn = lf.factory(name, 0.1, 0.3)
        assert fn.keywords == {'label_smoothing': 0.1, 'ctc_weight': 0.3}
        assert lf.factory(name, 0.1).keywords == {'label_smoothing': 0.1}
    assert lf.factory('CTC', ctc_weight=0.0) is lf.CTC
    for bad in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError, match='ctc_weight'):
            lf.factory('average_cross_entropy', ctc_weight=bad)


def test_no_shipped_recipe_or_defaults_file_sets_the_keys():
    for recipe in sorted(os.listdir(recipes.RECIPES)):
        d = os.path.join(recipes.RECIPES, recipe)
        if os.path.isdir(d):
            for name in os.listdir(d):
                assert not re.search(r'^\s*ctc_(head|weight)\s*=', open(os.path.join(d, name)).read(), flags=re.M), name
    found = 0
    for dp, _, files in os.walk(os.path.join(ROOT, 'nabu_amd')):
        if os.path.basename(dp) == 'defaults':
            for name in files:
                found += 1
                assert not re.search(r'^\s*ctc_(head|weight)\s*=', open(os.path.join(dp, name)).read(), flags=re.M), name
    assert found > 10


def test_the_evaluator_asks_for_the_plain_loss():
    import inspect
    from nabu_amd.neuralnetworks.evaluators import loss_evaluator
    assert "loss_functions.factory(self.conf['loss'])(" in inspect.getsource(loss_evaluator.LossEvaluator.update_loss)


# ------------------------------------------------------------------------------------------------- call order: loss
def _fake_losses(monkeypatch, calls):
    from nabu_amd import ops as hip

    def xent(name):
        def fn(logits, targets, ll, tl, scale, *smoothing):
            calls.append((name, tuple(logits.shape), scale) + smoothing)
            return torch.zeros(logits.shape[0]), torch.zeros_like(logits)
        return fn
    for name in ('xent_loss_grad', 'xent_wide_loss_grad', 'xent_smooth_loss_grad', 'xent_wide_smooth_loss_grad'):
        monkeypatch.setattr(hip, name, xent(name))

    def ctc(logits, ll, labels, tl, scale):
        calls.append(('ctc_loss_grad', tuple(logits.shape), tuple(labels.shape), tl.tolist(), scale))
        return torch.zeros(logits.shape[0]), torch.zeros_like(logits), torch.zeros(1, dtype=torch.int32)
    monkeypatch.setattr(hip, 'ctc_loss_grad', ctc)
    monkeypatch.setattr(hip, 'sum_', lambda x, scale=1.0: (x.sum() * scale).reshape(1))
    monkeypatch.setattr(hip, 'axpy_', lambda y, x, a=1.0: y.add_(a * x))


@pytest.mark.parametrize('loss', ['average_cross_entropy', 'sum_cross_entropy'])
def test_without_the_weight_the_losses_call_what_they_always_called(loss, monkeypatch):
    """a model WITH a head and a trainer without the key: the head's logits are beside the output and the loss does not
    look at them; with the key the attention term is scaled by (1 - w) / B, the CTC term by w / B on the targets
    without their end label, and its status word is queued"""
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.trainers import loss_functions as lf
    calls = []
    _fake_losses(monkeypatch, calls)
    monkeypatch.setattr(lf, 'pending_status', [])
    tl = SeqLen([3, 2], dev_tensor=torch.tensor([3, 2], dtype=torch.int32))
    el = SeqLen([7, 5], dev_tensor=torch.tensor([7, 5], dtype=torch.int32))
    logits = {'text': torch.zeros(2, 3, 40), 'text_ctc': torch.zeros(2, 7, 40)}
    targets = {'text': torch.zeros(2, 3, dtype=torch.int32)}
    sl = {'text': tl, 'text_ctc': el}
    lf.factory(loss)(targets, logits, sl, {'text': tl})
    assert calls == [('xent_loss_grad', (2, 3, 40), 0.5)] and lf.pending_status == []
    del calls[:]
    lf.factory(loss, 0.0, 0.0)(targets, logits, sl, {'text': tl})
    assert calls == [('xent_loss_grad', (2, 3, 40), 0.5)]
    del calls[:]
    lf.factory(loss, ctc_weight=0.25)(targets, logits, sl, {'text': tl})
    assert calls == [('xent_loss_grad', (2, 3, 40), 0.375), ('ctc_loss_grad', (2, 7, 40), (2, 3), [2, 1], 0.125)]
    assert len(lf.pending_status) == 1
    del calls[:]
    lf.factory(loss, 0.1, 0.25)(targets, logits, sl, {'text': tl})
    assert [c[0] for c in calls] == ['xent_smooth_loss_grad', 'ctc_loss_grad'] and calls[0][2:] == (0.375, 0.1)
    with pytest.raises(ValueError, match='CTC head'):
        lf.factory(loss, ctc_weight=0.25)(targets, {'text': logits['text']}, sl, {'text': tl})


# ---------------------------------------------------------------------------------------- call order: the decoder
class _Model(object):
    """what BeamSearchDecoder touches of a model, on the CPU"""

    def __init__(self, head):
        self.output_dims = {'text': 5}
        self.store = None
        self.calls = []
        model = self

        class Dec(object):
            scope = 'Speller'
            ctc_head = head

            def create_cell(self, encoded, lens, is_training):
                return 'cell'

            def ctc_logits(self, encoded, lens):
                model.calls.append('ctc_logits')
                return 'head logits', lens['features']
        self.decoder = Dec()

    def encoder(self, inputs, input_seq_length, is_training):
        return {'features': 'encoded'}, {'features': 'lengths'}


def _decoder_conf(**extra):
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': 'beam_search_decoder', 'alphabet': 'a b c d', 'max_steps': '4',
                                     'beam_width': '3', 'length_penalty': '0.0', 'temperature': '1.0',
                                     'visualize_alignments': 'False'}, **extra)})
    return conf


def test_beam_search_decoder_without_the_key_makes_the_call_it_always_made(monkeypatch):
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.decoders import beam_search_decoder as bsd
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    seen = []

    def fake(*args, **kw):
        seen.append((args, kw))
        return ('seqs', 'lengths', 'scores', None)
    monkeypatch.setattr(rnn_decoder, 'beam_search', fake)
    monkeypatch.setattr(vs, 'as_default', lambda store: vs.variable_scope('x'))
    plain = dict(beam_width=3, max_steps=4, length_penalty=0.0, temperature=1.0, with_alignments=False)
    for head in (False, True):
        model = _Model(head)
        dec = bsd.BeamSearchDecoder(_decoder_conf(), model)
        assert dec.ctc_weight == 0.0
        assert dec({'features': None}, {'features': None}) == {'text': ('seqs', 'lengths', 'scores', None)}
        assert seen.pop() == (('cell', ['encoded'], ['lengths']), plain) and model.calls == []
    model = _Model(True)
    dec = bsd.BeamSearchDecoder(_decoder_conf(ctc_weight='0.3'), model)
    dec({'features': None}, {'features': None})
    assert seen.pop() == (('cell', ['encoded'], ['lengths']), dict(plain, ctc_logits='head logits', ctc_weight=0.3))
    assert model.calls == ['ctc_logits']
    with pytest.raises(ValueError, match='ctc_head = True'):
        bsd.BeamSearchDecoder(_decoder_conf(ctc_weight='0.3'), _Model(False))
    for bad in ('1', '-0.5', 'nan', 'x'):
        with pytest.raises(ValueError, match='ctc_weight'):
            bsd.BeamSearchDecoder(_decoder_conf(ctc_weight=bad), _Model(True))


def test_beam_search_refuses_a_weight_without_logits_and_a_weight_out_of_range():
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    with pytest.raises(ValueError, match='ctc_logits'):
        rnn_decoder.beam_search(None, None, None, 3, 4, ctc_weight=0.3)
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError, match='ctc_weight'):
            rnn_decoder.beam_search(None, None, None, 3, 4, ctc_logits=torch.zeros(1, 2, 3), ctc_weight=bad)
