"""GPU parity of the transducer recipe's training step (decoder = transducer, loss = transducer) against the float64
model of tests/transducer_model_ref.py: the loss and EVERY variable's gradient of one step, with one and with two
prediction layers; four clip + Adam updates; repeated updates on one batch.  The recipe is shrunk as test_hip_model.py
shrinks cfg1 (16 encoder units, 16 prediction units, B 4, T 40, 2-5 labels); the bounds are that file's."""
import numpy as np
import pytest
import torch

from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests import transducer_model_ref as mr

pytestmark = pytest.mark.gpu
RECIPE = 'dblstm_transducer_timit'
SMALL = {'encoder.num_units': 16, 'decoder.num_units': 16, 'trainer.batch_size': 4}


def make_trainer(data, **over):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe(RECIPE, **dict(SMALL, **over))
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                               expdir=None, server=None, task_index=0)


def synthetic(seed):
    return SyntheticData(4, 40, 40, min_frames=25, min_labels=2, max_labels=5, time_reduction=1, seed=seed)


@pytest.mark.parametrize('layers', [1, 2])
def test_single_step_gradients_match_the_float64_model(layers):
    from nabu_amd.autodiff import Tape
    from nabu_amd.neuralnetworks.trainers import loss_functions
    data = synthetic(7)
    tr = make_trainer(data, **{'decoder.num_layers': layers})
    b = tr.to_device(data.batch(0))
    with Tape() as tape:
        logits, lsl = tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], True)
        loss = loss_functions.factory('transducer')(b['targets'], logits, lsl, b['target_seq_length'])
    assert sorted(logits) == ['text', 'text_pred']
    assert list(lsl['text_pred'].host) == list(data.batch(0)['target_seq_length']['text'] + 1)
    assert logits['text_pred'].shape == (4, data.batch(0)['targets']['text'].shape[1] + 1, 40)
    tape.backward(loss)
    loss_functions.check_status()
    names = [v.name for v in tr.model.variables]
    want = ['Transducer/text/transcription/weights', 'Transducer/text/transcription/biases']
    for l in range(layers):
        want += ['Transducer/text/prediction/layer%d/lstm_cell/kernel' % l, 'Transducer/text/prediction/layer%d/lstm_cell/bias' % l]
    want += ['Transducer/text/prediction/outlayer/weights', 'Transducer/text/prediction/outlayer/biases']
    assert [n for n in names if n.startswith('Transducer/')] == want
    P = mr.params_of(tr.model.store.state_dict())
    assert mr.counts(P) == (2, layers) and P[mr.PRED % 0 + 'kernel'].shape == (40 + 16, 64)
    ref_loss, G = mr.step(P, data.batch(0))
    assert abs(float(loss.item()) - ref_loss) / ref_loss < 1e-5, (float(loss.item()), ref_loss)
    assert sorted(G) == sorted(names)
    for v in tr.model.variables:
        got, ref = v.grad.cpu().numpy().astype(np.float64), G[v.name]
        assert got.shape == ref.shape and np.abs(ref).max() > 0, v.name
        err = np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12)
        print(v.name, 'gradient error %.2e of the largest entry' % err)
        assert err < 2e-4, (v.name, err)


def test_without_targets_only_the_transcription_logits_are_returned():
    data = synthetic(7)
    tr = make_trainer(data)
    b = tr.to_device(data.batch(0))
    with torch.no_grad():
        full, _ = tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)
        logits, lsl = tr.model(b['inputs'], b['input_seq_length'], [], [], False)
    assert list(logits) == ['text'] and list(lsl) == ['text'] and torch.equal(logits['text'], full['text'])
    assert len(tr.model.variables) == 8 + 6


def test_training_trajectory_matches_the_float64_model():
    data = synthetic(2234)
    tr = make_trainer(data)
    losses = [float(tr.step(tr.to_device(data.batch(s))).item()) for s in range(4)]
    tr2 = make_trainer(data)             # the same seed: the same initial weights
    b0 = tr2.to_device(data.batch(0))
    with torch.no_grad():
        tr2.model(b0['inputs'], b0['input_seq_length'], b0['targets'], b0['target_seq_length'], False)
    P = mr.params_of(tr2.model.store.state_dict())
    M, V, ref_losses = {}, {}, []
    for s in range(4):
        loss, G = mr.step(P, data.batch(s))
        ref_losses.append(loss)
        mr.adam(P, G, M, V, s + 1)
    rel = np.abs(np.array(losses) - np.array(ref_losses)) / np.abs(ref_losses)
    print('losses', losses, 'float64', ref_losses)
    assert rel.max() < 1e-3, (losses, ref_losses)
    assert rel.max() < 5e-5, (losses, ref_losses)
    got = mr.params_of(tr.model.store.state_dict())
    for k in P:               # (test_hip_model.py on these two bounds: the mean carries the check)
        d = np.abs(got[k] - P[k])
        assert d.max() < 4.5e-3 and d.mean() < 2e-5, (k, d.max(), d.mean())


def test_repeated_updates_on_one_batch_reduce_the_loss():
    data = synthetic(3)
    tr = make_trainer(data)
    b = tr.to_device(data.batch(0))
    ls = [float(tr.step(b).item()) for _ in range(20)]
    assert ls[-1] < ls[0] and all(np.isfinite(ls)), ls


def test_a_label_outside_the_classes_raises_the_transducer_message():
    data = synthetic(5)
    tr = make_trainer(data)
    batch = data.batch(0)
    batch['targets']['text'] = batch['targets']['text'].copy()
    batch['targets']['text'][2, 0] = 39                      # the blank's class
    from nabu_amd.neuralnetworks.trainers import loss_functions
    tr.step(tr.to_device(batch))
    with pytest.raises(Exception, match='transducer: invalid utterance 2 of the batch'):
        loss_functions.check_status()
