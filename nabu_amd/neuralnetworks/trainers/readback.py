"""When Trainer.train() reads a step's words from the device: at once (ReadNow, the reference's loop) or one step late
(ReadLate, prefetch_batches >= 1).

What the loop reads from the device after every step — the loss, one status word per CTC kernel
(loss_functions.pending_status) and the status word of every persistent-kernel workspace (ops.check_persist_status) —
lands, for the late read, in ONE pinned record per step: a few asynchronous copies on the launch stream, closed by an
event.  The record of step s is read after step s + 1 has been enqueued, so the host never waits for the step it has
just launched."""
import numpy as np
import torch

from nabu_amd import ops as hip
from nabu_amd.neuralnetworks.trainers import loss_functions

WORDS = 32          # 1 loss word + CTC status words (one per output and micro-batch) + one word per persistent-kernel
                    # workspace; a record that needs more grows by this many


class StepRecord(object):
    '''host words of one step: [0] the loss (float32 bits), [1 : 1 + n_ctc] the CTC status words, then one status word
    per workspace of `workspaces`'''

    def __init__(self, pinned=False):
        self.host = torch.zeros(WORDS, dtype=torch.int32, pin_memory=pinned)
        self.event = None
        self.step, self.n_ctc, self.workspaces, self.errors = None, 0, [], []

    def fill(self, step, loss, ctc_status, workspaces):
        '''enqueue the copies of this step's words behind the step (device tensors: asynchronous, closed by an event)'''
        need = 1 + len(ctc_status) + len(workspaces)
        if need > self.host.numel():       # an accumulated update brings the CTC words of all its micro-batches
            self.host = torch.zeros((need + WORDS - 1) // WORDS * WORDS, dtype=torch.int32, pin_memory=self.host.is_pinned())
        self.step, self.n_ctc, self.workspaces = step, len(ctc_status), list(workspaces)
        self.errors = [getattr(s, 'error', loss_functions.ctc_status_error) for s in ctc_status]    # what each word means
        self.host[0:1].view(torch.float32).copy_(loss.detach().reshape(1).to(torch.float32), non_blocking=True)
        for i, s in enumerate(ctc_status):
            self.host[1 + i:2 + i].copy_(s.reshape(1), non_blocking=True)
        for i, (tag, buf) in enumerate(self.workspaces):
            self.host[1 + self.n_ctc + i:2 + self.n_ctc + i].copy_(buf[:4].view(torch.int32), non_blocking=True)
        self.event = None
        if loss.is_cuda:
            self.event = torch.cuda.Event()
            self.event.record()
        return self

    def read(self):
        '''wait for the step and return its loss; raises what the synchronous loop raises for a non-zero status word,
        with the step it belongs to (a persistent kernel's word is cleared, as ops.check_persist_status clears it)'''
        if self.event is not None:
            self.event.synchronize()
            self.event = None
        words = self.host.numpy()
        for error, code in zip(self.errors, words[1:1 + self.n_ctc]):
            if code:
                raise Exception('%s [step %d]' % (error(int(code)), self.step))
        for (tag, buf), code in zip(self.workspaces, words[1 + self.n_ctc:]):
            if code:
                if buf is not None:
                    buf[:4].zero_()
                err = hip.persist_status_error(tag, int(code))
                raise type(err)('%s [step %d]' % (err, self.step))
        return float(words[0:1].view(np.float32)[0])


class ReadNow(object):
    '''lag 0: a step's status words are checked and its loss is read as soon as the step is enqueued.  `reduce(loss)`
    is the loss summed over the replicas (the status check precedes that collective), `report(step, loss_sum, lr,
    start)` takes what was read.'''
    lag = 0

    def __init__(self, reduce, report):
        self.reduce, self.report = reduce, report

    def push(self, step, loss, lr, start):
        loss_functions.check_status()
        self.report(step, float(self.reduce(loss).item()), lr, start)

    def drain(self, keep=0):
        pass


class ReadLate(ReadNow):
    '''lag 1: push() enqueues the copies of a step's words into a StepRecord, drain(keep) reads and reports all but the
    latest `keep` records — the loop keeps one while it runs and none before a validation point, before a checkpoint
    and at the end.  A non-zero status word raises when its record is read, naming its step.'''
    lag = 1

    def __init__(self, reduce, report, pinned):
        ReadNow.__init__(self, reduce, report)
        self.pinned, self.pending, self.spare = pinned, [], []     # records not read yet / read and free to reuse

    def push(self, step, loss, lr, start):
        loss = self.reduce(loss)
        rec = self.spare.pop() if self.spare else StepRecord(pinned=self.pinned)
        rec.fill(step, loss, loss_functions.take_pending_status(), hip.persist_workspaces())
        rec.lr, rec.start = lr, start
        self.pending.append(rec)

    def drain(self, keep=0):
        while len(self.pending) > keep:
            rec = self.pending.pop(0)
            self.report(rec.step, rec.read(), rec.lr, rec.start)
            self.spare.append(rec)
