"""GPU: Trainer.train with prefetch_batches = 2 (batches staged by worker threads, one upload and one unpack launch per
batch, losses and status words read one step late) against the synchronous loop on shrunken recipes: the same history,
validation history and final weights, bit for bit — also across an interrupted and resumed run — and an infeasible CTC
batch that raises one iteration late, naming its step."""
import os
import threading

import numpy as np
import pytest

from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData

pytestmark = pytest.mark.gpu

OVER = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.num_epochs': 1, 'trainer.valid_frequency': 3,
        'evaluator.batch_size': 2, 'evaluator.numbatches': 2}


def synthetic():
    return SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11,
                         batches_per_epoch=6)


def cfg2_trainer(prefetch, expdir=None, data=None):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **OVER)
    if prefetch is not None:
        tc.set('trainer', 'prefetch_batches', str(prefetch))
    return trainer_factory.factory('standard')(conf=tc, dataconf=data or synthetic(), modelconf=mc, evaluatorconf=ec,
                                               expdir=expdir, server=None, task_index=0)


def workers():
    return [t for t in threading.enumerate() if t.name.startswith('nabu-prefetch')]


def assert_same_run(a, hist_a, b, hist_b):
    assert [h[0] for h in hist_a] == [h[0] for h in hist_b] and len(hist_a) >= 6
    np.testing.assert_array_equal(np.array([h[1] for h in hist_a]), np.array([h[1] for h in hist_b]))
    assert [h[2] for h in hist_a] == [h[2] for h in hist_b]
    assert a.validation_history == b.validation_history and len(a.validation_history) >= 2
    sa, sb = a.model.store.state_dict(), b.model.store.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k])


@pytest.fixture(scope='module')
def synchronous_run():
    tr = cfg2_trainer(None)
    return tr, tr.train()


def test_cfg2_synthetic_equals_the_synchronous_loop(synchronous_run):
    want, want_hist = synchronous_run
    got = cfg2_trainer(2)
    got_hist = got.train()
    assert workers() == []
    assert all(np.isfinite(h[1]) for h in got_hist)
    assert_same_run(got, got_hist, want, want_hist)


def test_interrupted_and_resumed_run_equals_the_synchronous_loop(synchronous_run, tmp_path):
    want, want_hist = synchronous_run
    part = cfg2_trainer(2, str(tmp_path / 'part'))
    part.checkpoint_steps = 3
    orig = type(part).step
    calls = {'n': 0}

    class Stop(Exception):
        pass

    def step_then_stop(self, batch):
        if calls['n'] == 3:
            raise Stop()
        calls['n'] += 1
        return orig(self, batch)
    type(part).step = step_then_stop
    try:
        with pytest.raises(Stop):
            part.train()
    finally:
        type(part).step = orig
    assert workers() == []
    assert os.path.exists(str(tmp_path / 'part' / 'logdir' / 'model.ckpt'))
    cont = cfg2_trainer(2, str(tmp_path / 'part'))
    hist = cont.train()
    assert workers() == []
    assert [h[0] for h in hist] == [3, 4, 5]
    np.testing.assert_array_equal(np.array([h[1] for h in hist]), np.array([h[1] for h in want_hist[3:]]))
    assert cont.validation_history == want.validation_history[1:]
    a, b = want.model.store.state_dict(), cont.model.store.state_dict()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_cfg1_tfrecord_buckets_equal_the_synchronous_loop(tmp_path):
    from tests.test_data_path import make_dataset
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    conf, _, _, _ = make_dataset(str(tmp_path / 'train'), n=24, dim=40, min_frames=14)
    dev, _, _, _ = make_dataset(str(tmp_path / 'dev'), n=6, dim=40, seed=5, min_frames=14)
    conf.read_dict({'devfbank': dict(dev.items('trainfbank')), 'devtext': dict(dev.items('traintext'))})

    def run(prefetch):
        mc, tc, ec = recipes.load_recipe('cfg1_dblstm_ctc', **{
            'encoder.num_units': 16, 'trainer.batch_size': 4, 'trainer.numbuckets': 2, 'trainer.num_epochs': 1,
            'trainer.valid_frequency': 3, 'evaluator.batch_size': 2, 'io.output_dims': 4})
        tc.set('trainer', 'features', 'trainfbank')
        tc.set('trainer', 'targets', 'text')
        tc.set('trainer', 'text', 'traintext')
        if prefetch:
            tc.set('trainer', 'prefetch_batches', str(prefetch))
            tc.set('trainer', 'prefetch_workers', '3')
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=conf, modelconf=mc, evaluatorconf=ec,
                                                 expdir=None, server=None, task_index=0)
        hist = tr.train()
        tr.data.close()
        return tr, hist
    want, want_hist = run(0)
    got, got_hist = run(2)
    assert workers() == []
    assert len(got_hist) == got.data.num_batches() and all(np.isfinite(h[1]) for h in got_hist)
    assert_same_run(got, got_hist, want, want_hist)


class OneBadBatch(object):
    """the synthetic source with a CTC target that cannot fit its frames in batch `bad`"""

    def __init__(self, bad):
        self.data, self.bad = synthetic(), bad

    def num_batches(self):
        return self.data.num_batches()

    def validation(self, *args, **kwargs):
        return self.data.validation(*args, **kwargs)

    def batch(self, step):
        b = self.data.batch(step)
        if step == self.bad:
            b['targets']['text'] = np.zeros_like(b['targets']['text'])      # 3 repeats need 5 frames, the encoder has 4
            b['target_seq_length']['text'] = np.full_like(b['target_seq_length']['text'], 3)
        return b


@pytest.mark.parametrize('prefetch, enqueued', [(0, 2), (2, 3)])
def test_infeasible_ctc_batch_raises_one_iteration_late(prefetch, enqueued):
    """a status code of the loss kernel: the synchronous loop raises after step 1, the overlapped loop after it has
    enqueued step 2, and names the step"""
    tr = cfg2_trainer(prefetch, data=OneBadBatch(1))
    orig = type(tr).step
    steps = []

    def counted(self, batch):
        steps.append(self.global_step)
        return orig(self, batch)
    type(tr).step = counted
    try:
        with pytest.raises(Exception, match='Not enough time for target transition sequence' +
                                            (r'.*\[step 1\]' if prefetch else '')):
            tr.train()
    finally:
        type(tr).step = orig
    assert steps == list(range(enqueued))
    assert workers() == []
    from nabu_amd.neuralnetworks.trainers import loss_functions
    loss_functions.take_pending_status()                # (the step enqueued behind the bad one left its word pending)
    loss_functions.check_status()                       # no persistent kernel gave up: a status code, not a fault
