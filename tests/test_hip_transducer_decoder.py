"""TransducerDecoder (greedy lock-step search on the device) against the restatement's greedy search on the model's
float64 forward pass (tests/transducer_model_ref.py).

The model of test_hip_transducer_model.py is trained for 30 updates on one batch (learning rate 0.06: at the recipe's
1e-3 thirty updates teach it the blank and nothing else).  Before anything is compared the test asserts a CONDITION on
the restatement alone — every decision along the reference's path is clear by at least 1e-3 in the joint logits, every
utterance's path has a blank and an emission, some frame emits twice — so that equality of the ids is a fair demand
on float32 and the comparison is not vacuous.  Seed and rate were chosen on the CPU, by running the float64 model's
own updates from the same initial weights; if the condition fails, the test fails."""
import configparser

import numpy as np
import pytest
import torch

from nabu_amd import ops, recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests import transducer_model_ref as mr

pytestmark = pytest.mark.gpu
RECIPE = 'dblstm_transducer_timit'
SEED, RATE, UPDATES, MAX_STEPS = 0, 0.06, 30, 10
ALPHABET = ' '.join('p%d' % i for i in range(39))
OVER = {'encoder.num_units': 16, 'decoder.num_units': 16, 'trainer.batch_size': 4, 'trainer.initial_learning_rate': RATE,
        'decoder.max_steps': MAX_STEPS, 'decoder.text_alphabet': ALPHABET, 'evaluator.batch_size': 4,
        'evaluator.numbatches': 2}
_trained = {}


def trained():
    """(trainer, data, the batch it was trained on): built once for the tests of this file"""
    if not _trained:
        from nabu_amd.neuralnetworks.trainers import trainer_factory
        data = SyntheticData(4, 40, 40, min_frames=25, min_labels=2, max_labels=5, time_reduction=1, seed=SEED)
        mc, tc, ec = recipes.load_recipe(RECIPE, **OVER)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                 server=None, task_index=0)
        b = tr.to_device(data.batch(0))
        losses = [float(tr.step(b).item()) for _ in range(UPDATES)]
        _trained.update(tr=tr, data=data, ec=ec, losses=losses)
    return _trained['tr'], _trained['data'], _trained['ec']


def decoder_of(tr, **extra):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': 'transducer_decoder', 'max_steps': str(MAX_STEPS), 'text_alphabet': ALPHABET},
                                    **extra)})
    return decoder_factory.factory('transducer_decoder')(conf, tr.model)


def test_greedy_search_equals_the_restatement_on_the_float64_forward_pass(tmp_path):
    tr, data, _ = trained()
    batch = data.batch(0)
    P = mr.params_of(tr.model.store.state_dict())
    ids64, len64, pos64, score64, margins, paths, f64, el = mr.greedy(P, batch['inputs']['features'],
                                                                    batch['input_seq_length']['features'], MAX_STEPS)
    blank = f64.shape[2] - 1
    # the CONDITION, on the restatement alone
    worst = min(min(m) for m in margins)
    print('losses %.3f -> %.3f, smallest margin %.3e, lengths %s, frames %s' % (_trained['losses'][0], _trained['losses'][-1],
                                                                              worst, len64, pos64))
    assert worst >= 1e-3, worst
    for b, path in enumerate(paths):
        assert any(k == blank for _, k in path) and any(k != blank for _, k in path), (b, path)
    per_row = [[t for t, k in path if k != blank] for path in paths]
    assert any(len(ts) != len(set(ts)) for ts in per_row), per_row          # some frame emits twice
    assert np.all(len64 < MAX_STEPS) and np.array_equal(pos64, el)           # (every row ends by running out of frames)

    dec = decoder_of(tr)
    b = tr.to_device(batch)
    out = dec(b['inputs'], b['input_seq_length'])
    assert list(out) == ['text']
    ids, lens = out['text']
    assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and tuple(ids.shape) == (4, MAX_STEPS)
    assert np.array_equal(lens.cpu().numpy(), len64), (lens.cpu().numpy(), len64)
    assert np.array_equal(ids.cpu().numpy(), ids64), (ids.cpu().numpy(), ids64)
    assert np.allclose(dec.scores['text'].cpu().numpy(), score64, rtol=1e-4, atol=1e-4)
    again = dec(b['inputs'], b['input_seq_length'])['text']
    assert torch.equal(again[0], ids) and torch.equal(again[1], lens)

    # write: one line per utterance; the error rate: ops.edit_distance on the same ids
    names = ['utt%d' % i for i in range(4)]
    dec.write(out, str(tmp_path), names)
    lines = open(str(tmp_path / 'text')).read().splitlines()
    assert lines == ['%s %s' % (n, ' '.join('p%d' % j for j in ids64[i, :len64[i]])) for i, n in enumerate(names)]
    ref, ref_len = batch['targets']['text'], batch['target_seq_length']['text']
    dist = ops.edit_distance(ids, lens, torch.as_tensor(ref).to(torch.int32).cuda(), torch.as_tensor(ref_len).to(torch.int32).cuda())
    loss = [0.0]
    dec.reset()
    dec.update_evaluation_loss(loss, out, {'text': ref}, {'text': ref_len})
    assert loss[0] == float(dist.sum().item()) / float(ref_len.sum()) and 0 < loss[0] < 2


def test_a_row_that_reaches_max_steps_stops_there():
    tr, data, _ = trained()
    batch = data.batch(0)
    P = mr.params_of(tr.model.store.state_dict())
    ids64, len64 = mr.greedy(P, batch['inputs']['features'], batch['input_seq_length']['features'], 1)[:2]
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': {'decoder': 'transducer_decoder', 'max_steps': '1', 'text_alphabet': ALPHABET}})
    dec = decoder_factory.factory('transducer_decoder')(conf, tr.model)
    b = tr.to_device(batch)
    ids, lens = dec(b['inputs'], b['input_seq_length'])['text']
    assert np.array_equal(ids.cpu().numpy(), ids64) and np.array_equal(lens.cpu().numpy(), len64) and np.all(len64 == 1)


def test_decoder_evaluator_runs_the_search_over_the_validation_batches():
    """a `run test`-style pass: the recipe's evaluator conf (decoder_evaluator + transducer_decoder) through
    DecoderEvaluator on the synthetic validation set"""
    from nabu_amd.neuralnetworks.evaluators import evaluator_factory
    tr, data, ec = trained()
    ev = evaluator_factory.factory('decoder_evaluator')(ec, data, tr.model)
    loss, update, n = ev.evaluate()
    assert n == 2
    for i in range(n):
        update(i)
    assert np.isfinite(loss[0]) and 0 < loss[0] < 10
    assert ev.decoder.num_targets > 0


def test_refusals():
    tr, _, _ = trained()
    for key in ('lm_file', 'ctc_weight', 'timestamps'):
        with pytest.raises(ValueError, match=key):
            decoder_of(tr, **{key: '1'})
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe('cfg1_dblstm_ctc', **{'encoder.num_units': 16, 'trainer.batch_size': 4})
    ctc = trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(4, 40, 40), modelconf=mc, evaluatorconf=ec,
                                              expdir=None, server=None, task_index=0)
    with pytest.raises(ValueError, match='decoder = transducer'):
        decoder_of(ctc)
