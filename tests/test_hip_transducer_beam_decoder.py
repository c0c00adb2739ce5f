"""TransducerDecoder with beam_width (the alignment-length synchronous beam search on the device) against the
restatement's beam search on the model's float64 forward pass (tests/transducer_beam_ref.py on
tests/transducer_model_ref.py).

The model is trained as in test_hip_transducer_decoder.py — this file's own copy of that set-up: 30 updates on one
batch, units 16, B 4.  Before anything is compared the test asserts CONDITIONS on the restatement alone: the smallest
selection margin is at least 1e-3, so that equal labels are a fair demand on float32; some candidates merge; and the
beam's best hypothesis differs from the greedy result on some utterance, or beats its score.  The data seed was chosen
among 0 .. 6 by the restatement's margin on the float64 forward pass after 30, 35 and 40 updates (seed 2 after 30 has
1.1e-2, ten times the demand; seed 0, that file's, has 3.3e-4); if a condition fails, the test fails."""
import configparser

import numpy as np
import pytest
import torch

from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests import transducer_beam_ref as br
from tests import transducer_model_ref as mr

pytestmark = pytest.mark.gpu
RECIPE = 'dblstm_transducer_timit'
SEED, RATE, UPDATES, MAX_STEPS, WIDTH = 2, 0.06, 30, 10, 4
ALPHABET = ' '.join('p%d' % i for i in range(39))
OVER = {'encoder.num_units': 16, 'decoder.num_units': 16, 'trainer.batch_size': 4, 'trainer.initial_learning_rate': RATE,
        'decoder.max_steps': MAX_STEPS, 'decoder.text_alphabet': ALPHABET, 'evaluator.batch_size': 4,
        'evaluator.numbatches': 2}
_trained = {}


def trained():
    """(trainer, data, evaluator conf): built once for the tests of this file"""
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


def reference(P, x, lens, S, W):
    """the restatement's beam search and greedy search on the float64 forward pass"""
    f, el, _ = mr.transcription(P, x, lens)
    C = f.shape[2]
    cache = {}

    def g_fn(b, y):                       # (the prediction network does not see the utterance)
        y = tuple(int(k) for k in y)
        if y not in cache:
            hist = np.array([(C - 1,) + y], np.int64)
            cache[y] = mr.prediction(P, hist, [hist.shape[1]])[0][0, -1]
        return cache[y]
    res = br.beam_search(f, el, S, W, g_fn)
    greedy = mr.greedy(P, x, lens, S)
    return res, greedy


def test_beam_search_equals_the_restatement_on_the_float64_forward_pass(tmp_path):
    tr, data, _ = trained()
    batch = data.batch(0)
    P = mr.params_of(tr.model.store.state_dict())
    res, greedy = reference(P, batch['inputs']['features'], batch['input_seq_length']['features'], MAX_STEPS, WIDTH)
    ids64, len64, score64 = br.best(res['finals'], MAX_STEPS)
    g_ids, g_len, _, g_score = greedy[:4]
    # the CONDITIONS, on the restatement alone
    differs = [b for b in range(4) if not np.array_equal(ids64[b], g_ids[b])]
    beats = [b for b in range(4) if score64[b] > g_score[b] + 1e-3]
    print('losses %.3f -> %.3f, smallest margin %.3e, merges %s, lengths %s (greedy %s), differs on %s, beats on %s' %
          (_trained['losses'][0], _trained['losses'][-1], res['margin'], res['merges'], len64, g_len, differs, beats))
    print('scores', score64, 'greedy', g_score)
    assert res['margin'] >= 1e-3, res['margin']
    assert sum(res['merges']) >= 1
    assert differs or beats

    dec = decoder_of(tr, beam_width=str(WIDTH))
    b = tr.to_device(batch)
    out = dec(b['inputs'], b['input_seq_length'])
    assert list(out) == ['text']
    ids, lens = out['text']
    assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and tuple(ids.shape) == (4, MAX_STEPS)
    assert np.array_equal(lens.cpu().numpy(), len64), (lens.cpu().numpy(), len64)
    assert np.array_equal(ids.cpu().numpy(), ids64), (ids.cpu().numpy(), ids64)
    assert np.allclose(dec.scores['text'].cpu().numpy(), score64, rtol=1e-4, atol=1e-4)
    n_ids, n_len, n_score = (t.cpu().numpy() for t in dec.nbest['text'])
    assert n_ids.shape == (4, WIDTH, MAX_STEPS) and n_len.shape == n_score.shape == (4, WIDTH)
    for u, fin in enumerate(res['finals']):
        assert n_len[u].tolist() == [len(y) for y, _ in fin] + [-1] * (WIDTH - len(fin)), (u, n_len[u], fin)
        for j, (y, s) in enumerate(fin):
            assert n_ids[u, j, :len(y)].tolist() == list(y) and np.all(n_ids[u, j, len(y):] == -1), (u, j)
            assert abs(n_score[u, j] - s) <= 1e-4 + 1e-4 * abs(s), (u, j, n_score[u, j], s)
    again = dec(b['inputs'], b['input_seq_length'])['text']
    assert torch.equal(again[0], ids) and torch.equal(again[1], lens)

    # write: one line per utterance, the format of the greedy search's files
    names = ['utt%d' % i for i in range(4)]
    dec.write(out, str(tmp_path), names)
    lines = open(str(tmp_path / 'text')).read().splitlines()
    assert lines == ['%s %s' % (n, ' '.join('p%d' % j for j in ids64[i, :len64[i]])) for i, n in enumerate(names)]


def test_a_beam_of_one_and_no_key_give_the_greedy_outputs_bit_for_bit():
    tr, data, _ = trained()
    b = tr.to_device(data.batch(0))
    plain, one = decoder_of(tr), decoder_of(tr, beam_width='1')
    assert plain.beam_width == one.beam_width == 1
    (ids, lens), (ids1, lens1) = plain(b['inputs'], b['input_seq_length'])['text'], one(b['inputs'], b['input_seq_length'])['text']
    assert torch.equal(ids, ids1) and torch.equal(lens, lens1)
    assert plain.scores['text'].cpu().numpy().tobytes() == one.scores['text'].cpu().numpy().tobytes()
    assert plain.nbest == {} and one.nbest == {}


def test_decoder_evaluator_runs_the_beam_search():
    from nabu_amd.neuralnetworks.evaluators import evaluator_factory
    tr, data, _ = trained()
    _, _, ec = recipes.load_recipe(RECIPE, **dict(OVER, **{'decoder.beam_width': str(WIDTH)}))
    ev = evaluator_factory.factory('decoder_evaluator')(ec, data, tr.model)
    assert ev.decoder.beam_width == WIDTH
    loss, update, n = ev.evaluate()
    assert n == 2
    for i in range(n):
        update(i)
    assert np.isfinite(loss[0]) and 0 < loss[0] < 10
    assert ev.decoder.num_targets > 0


def test_refusals():
    tr, _, _ = trained()
    for bad in ('0', '33', 'x', '-2', '2.5'):
        with pytest.raises(ValueError, match='beam_width'):
            decoder_of(tr, beam_width=bad)
    for key in ('lm_file', 'ctc_weight', 'timestamps'):
        with pytest.raises(ValueError, match=key):
            decoder_of(tr, beam_width='4', **{key: '1'})
