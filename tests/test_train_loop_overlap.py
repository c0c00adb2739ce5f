"""CPU: Trainer.train with prefetch_batches = 2 against the synchronous loop, on the stubbed trainer of
tests/test_validation_loop.py (fake step, scripted validation loss, identity stage / to_device_staged): same history,
validation history and final state; and, from an event log, the ordering the overlapped loop exists for."""
import threading

import numpy as np
import pytest
import torch

from tests import test_validation_loop as base

SCRIPTS = {
    'plain': ([5.0, 4.0, 3.0, 2.0], dict(valid_frequency=4, num_tries='None')),
    'early_stopping': ([5.0, 6.0, 7.0, 8.0], dict(valid_frequency=2, num_tries=2, reset_tries='True')),
    'go_back': ([5.0, 6.0, 4.0, 4.5, 1.0, 0.9], dict(valid_frequency=3, num_tries='None', go_back='True',
                                                     valid_adapt='True')),
}


class LoggedLoss(object):
    """stands for the device loss: the log shows when the loop reads it"""

    def __init__(self, value, step, log):
        self.value, self.step, self.log = torch.tensor([value]), step, log
        self.is_cuda = False

    def detach(self):
        return self.value

    def item(self):
        self.log.append(('read', self.step))
        return self.value.item()


class StandardTrainer(base.StandardTrainer):
    """(same class name: the defaults file is looked up by it)"""

    def __init__(self, script, **over):
        super().__init__(script, **over)
        self.log = []
        data, log = self.dataconf, self.log

        class Source(object):
            def num_batches(self):
                return data.num_batches()

            def validation(self, *args, **kwargs):
                return data.validation(*args, **kwargs)

            def batch(self, step):
                log.append(('request', step))
                return {'step': step, 'batch': data.batch(step)}
        self.dataconf = Source()

    def stage(self, batch, slot=None):
        self.log.append(('stage', batch['step'], threading.current_thread() is threading.main_thread()))
        return batch

    def to_device_staged(self, staged):
        return staged

    def step(self, batch):
        self.log.append(('step', batch['step']))
        return LoggedLoss(float(super().step(batch)), batch['step'], self.log)


def run(script, prefetch, **over):
    over = dict(over, prefetch_batches=prefetch) if prefetch is not None else over
    tr = StandardTrainer(script, **{'trainer.' + k: v for k, v in over.items()})
    hist = tr.train()
    assert [t for t in threading.enumerate() if t.name.startswith('nabu-prefetch')] == []
    return tr, hist


@pytest.mark.parametrize('name', sorted(SCRIPTS))
def test_overlapped_loop_equals_the_synchronous_loop(name):
    script, over = SCRIPTS[name]
    want, want_hist = run(script, None, **over)
    zero, zero_hist = run(script, 0, **over)
    got, got_hist = run(script, 2, **over)
    assert len(want_hist) >= 6 and got_hist == want_hist == zero_hist
    for a in (zero, got):
        assert a.validation_history == want.validation_history
        assert (a.global_step, a.learning_rate_fact, a.weights, a.best_validation, a.num_tries) == \
            (want.global_step, want.learning_rate_fact, want.weights, want.best_validation, want.num_tries)
    # the synchronous loop reads every loss before it asks for the next batch and never calls stage
    assert not [e for e in want.log if e[0] == 'stage'] and not [e for e in zero.log if e[0] == 'stage']


def test_batches_are_requested_ahead_and_losses_read_one_step_late(monkeypatch):
    from nabu_amd.neuralnetworks.trainers import readback
    script, over = SCRIPTS['go_back']
    tr = StandardTrainer(script, **{'trainer.' + k: v for k, v in dict(over, prefetch_batches=2).items()})
    read = readback.StepRecord.read

    def logged_read(self):
        tr.log.append(('read', self.step))                     # the host waits for the step's record here
        return read(self)
    monkeypatch.setattr(readback.StepRecord, 'read', logged_read)
    hist = tr.train()
    log = tr.log
    at = {}
    for i, e in enumerate(log):
        at.setdefault(e[:2], []).append(i)
    assert all(not on_main for kind, _, on_main in [e for e in log if e[0] == 'stage'])
    assert len([e for e in log if e[0] == 'stage']) >= len(hist)
    steps = [e[1] for e in log if e[0] == 'step']
    assert steps == [h[0] for h in hist]                       # every batch that reached step() is its global step's
    reads = [e[1] for e in log if e[0] == 'read']
    assert reads == steps                                      # every loss is read once, in order
    for n, k in enumerate(steps[:-1]):
        i_read = [i for i in at[('read', k)]][steps[:n + 1].count(k) - 1]
        # batch k + 1 had been requested, and (unless a validation point drained the loop) step k + 1 enqueued
        assert min(at[('request', k + 1)]) < i_read
        nxt = steps[n + 1]
        if nxt == k + 1 and (k + 1) % 3 != 0:
            i_next = at[('step', nxt)][steps[:n + 2].count(nxt) - 1]
            assert i_next < i_read, 'the loss of step %d was read before step %d was enqueued' % (k, nxt)
    # go-back at step 3 to step 0 and at step 6 to step 3: nothing staged for the abandoned steps reached step()
    assert steps == [0, 1, 2, 0, 1, 2, 3, 4, 5, 3, 4, 5, 6, 7, 8, 9, 10, 11]


def test_a_status_word_in_a_record_raises_with_its_step():
    """the plumbing of the late errors, on the host side of a record: a CTC status word and a persistent kernel's
    time-out word raise today's text plus the step; the workspace word is cleared"""
    from nabu_amd import _hip
    from nabu_amd.neuralnetworks.trainers.readback import StepRecord
    rec = StepRecord().fill(7, torch.tensor([1.5]), [torch.tensor([0], dtype=torch.int32)], [])
    assert rec.read() == 1.5
    rec = StepRecord().fill(7, torch.tensor([1.5]), [torch.tensor([0], dtype=torch.int32),
                                                     torch.tensor([3], dtype=torch.int32)], [])
    with pytest.raises(Exception, match=r'Not enough time for target transition sequence \(utterance 2 of the batch\) '
                                        r'\[step 7\]'):
        rec.read()
    ws = torch.zeros(256, dtype=torch.uint8)
    rec = StepRecord().fill(9, torch.tensor([2.0]), [], [('blstm', ws), ('speller', ws)])
    assert rec.read() == 2.0
    ws[:4].view(torch.int32)[0] = 4 * 5 + 2                     # what a kernel that gave up leaves: block 5, backward pass
    rec = StepRecord().fill(9, torch.tensor([2.0]), [], [('blstm', ws)])
    with pytest.raises(_hip.NabuHipError, match=r'persistent LSTM kernel timed out .*block 5, backward pass.* \[step 9\]'):
        rec.read()
    assert int(ws[:4].view(torch.int32)[0]) == 0
    # a word written into the record itself (no device involved)
    rec = StepRecord().fill(11, torch.tensor([2.0]), [], [('speller', ws)])
    rec.host[1] = 4 * 2 + 1
    with pytest.raises(_hip.NabuHipError, match=r'persistent decoder kernel .*block 2, forward pass.* \[step 11\]'):
        rec.read()
    assert np.isfinite(rec.host.numpy()[0:1].view(np.float32)[0])
