"""CPU: the ordered kernel and collective calls of ONE update, driven through Trainer._backward_and_update with the
float64 stand-ins of tests/test_grad_accum.py: A in {1, 3} x {one replica, two replicas flat, two replicas bucketed} x
{clean, after _add_weight_noise}.  Every expected list is written out below; a buffer is named by the trainer field it
is (a part of), an Adam call carries its gradient scale."""
import pytest
import torch

from tests import test_grad_accum as accum

N = 20
BUCKETS = ((0, 8), (8, 20))
G, ACC, CLEAN = 'flat_grad', 'flat_acc', 'flat_clean'
G0, G1, ACC0, ACC1 = 'flat_grad[0:8]', 'flat_grad[8:20]', 'flat_acc[0:8]', 'flat_acc[8:20]'
NOISE = ('weight_noise', 'flat', CLEAN)
FIRST = ('clip_accumulate', ACC, None, G)                # (out, acc, g)
NEXT = ('clip_accumulate', ACC, ACC, G)

EXPECTED = {
    # (A, exchange, noisy): the calls of one update, in order
    (1, 'none', False): [('adam_clip_step', 1.0)],
    (1, 'none', True): [NOISE, ('adam_clip_step_from', CLEAN, 1.0)],
    (1, 'flat', False): [('clip_', G), ('all_reduce_sum_', G), ('adam_clip_step', 1 / 2)],
    (1, 'flat', True): [NOISE, ('clip_', G), ('all_reduce_sum_', G), ('adam_clip_step_from', CLEAN, 1 / 2)],
    (1, 'bucketed', False): [('clip_', G0), ('all_reduce_sum_async', G0), ('clip_', G1), ('all_reduce_sum_async', G1),
                             ('adam_clip_step', 1 / 2)],
    (1, 'bucketed', True): [NOISE, ('clip_', G0), ('all_reduce_sum_async', G0), ('clip_', G1),
                            ('all_reduce_sum_async', G1), ('adam_clip_step_from', CLEAN, 1 / 2)],
    (3, 'none', False): [FIRST, NEXT, ('adam_clip_step_acc', None, ACC, G, 1 / 3)],            # (src, acc, g, scale)
    (3, 'none', True): [NOISE, FIRST, NEXT, ('adam_clip_step_acc', CLEAN, ACC, G, 1 / 3)],
    (3, 'flat', False): [FIRST, NEXT, ('clip_accumulate', G, ACC, G), ('all_reduce_sum_', G), ('adam_clip_step', 1 / 6)],
    (3, 'flat', True): [NOISE, FIRST, NEXT, ('clip_accumulate', G, ACC, G), ('all_reduce_sum_', G),
                        ('adam_clip_step_from', CLEAN, 1 / 6)],
    (3, 'bucketed', False): [FIRST, NEXT, ('clip_accumulate', G0, ACC0, G0), ('all_reduce_sum_async', G0),
                             ('clip_accumulate', G1, ACC1, G1), ('all_reduce_sum_async', G1), ('adam_clip_step', 1 / 6)],
    (3, 'bucketed', True): [NOISE, FIRST, NEXT, ('clip_accumulate', G0, ACC0, G0), ('all_reduce_sum_async', G0),
                            ('clip_accumulate', G1, ACC1, G1), ('all_reduce_sum_async', G1),
                            ('adam_clip_step_from', CLEAN, 1 / 6)],
}


class LoggingServer(accum.FakeServer):
    """FakeServer that names the buffer of every collective, the asynchronous ones included"""

    def __init__(self, world, log, name):
        super().__init__(world)
        self.log, self.name = log, name

    def all_reduce_sum_(self, t):
        self.log.append(('all_reduce_sum_', self.name(t)))
        return super().all_reduce_sum_(t)

    def all_reduce_sum_async(self, t):
        self.log.append(('all_reduce_sum_async', self.name(t)))
        t.mul_(self.world_size)
        return None                                              # (nothing in flight to wait for)


def logged_stand_ins(monkeypatch, log, name):
    """the stand-ins of test_grad_accum, each logging its buffers (and the gradient scale of an Adam call) first"""
    from nabu_amd import ops as hip
    S = accum.STAND_INS
    entries = {
        'clip_': lambda g, clip=1.0: ('clip_', name(g)),
        'clip_accumulate': lambda out, acc, g, clip=1.0: ('clip_accumulate', name(out), name(acc), name(g)),
        'adam_clip_step': lambda p, g, *a: ('adam_clip_step', a[-1]),
        'adam_clip_step_from': lambda p, src, g, *a: ('adam_clip_step_from', name(src), a[-1]),
        'adam_clip_step_acc': lambda p, src, acc, g, *a: ('adam_clip_step_acc', name(src), name(acc), name(g), a[-1]),
    }
    for fn_name, entry in entries.items():
        def logged(*a, _fn=S[fn_name], _entry=entry):
            log.append(_entry(*a))
            return _fn(*a)
        monkeypatch.setattr(hip, fn_name, logged)

    def weight_noise(flat, clean, table, stddev, seed, offset):
        log.append(('weight_noise', name(flat), name(clean)))
        clean.copy_(flat)
        flat.add_(stddev)
    monkeypatch.setattr(hip, 'weight_noise', weight_noise)
    monkeypatch.setattr(hip, 'set_phase_hook', lambda fn: None)  # (no recurrent kernel here calls a hook)


@pytest.mark.parametrize('noisy', [False, True])
@pytest.mark.parametrize('exchange', ['none', 'flat', 'bucketed'])
@pytest.mark.parametrize('A', [1, 3])
def test_the_calls_of_one_update(A, exchange, noisy, monkeypatch):
    from nabu_amd.autodiff import Tape, record
    log = []

    def name(t):
        if t is None:
            return None
        for field in ('flat_grad', 'flat_acc', 'flat_clean', 'flat'):
            base = getattr(tr, field)
            if base is not None and t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr():
                lo = t.storage_offset() - base.storage_offset()
                whole = lo == 0 and t.numel() == base.numel()
                return field if whole else '%s[%d:%d]' % (field, lo, lo + t.numel())
        raise AssertionError('a buffer that is none of the trainer\'s')

    logged_stand_ins(monkeypatch, log, name)
    world = 1 if exchange == 'none' else 2
    over = {accum.KEY: A * world}
    if noisy:
        over['trainer.weight_noise'] = 0.125
    tr = accum.make_trainer(LoggingServer(world, log, name) if world > 1 else None, **over)
    tr._create_graph()
    assert (tr.accumulate, tr.world) == (A, world)
    accum.seed_optimizer(tr, torch.linspace(-1, 1, N, dtype=torch.float64).numpy())
    tr.flat_grad = torch.zeros(N, dtype=torch.float64)
    if exchange == 'bucketed':             # two ranges of the gradient buffer; nothing declares their variables, so
        tr.buckets = [dict(key='b%d' % i, start=lo, end=hi, vars=[object()])      # both leave after the backward pass
                      for i, (lo, hi) in enumerate(BUCKETS)]
    if noisy:
        from nabu_amd.neuralnetworks.components import ops as nops
        monkeypatch.setattr(nops.global_rng(), 'offset', nops.global_rng().offset)     # (the draw's offset is given back)
        tr.flat_clean, tr.noise_table = torch.empty_like(tr.flat), None
        tr._add_weight_noise(None)
        assert tr._noisy
    before = tr.flat_clean.clone() if noisy else tr.flat.clone()
    for j in range(A):
        def backward(gout, value=0.25 * (j + 1)):                # the backward pass leaves its gradient in flat_grad
            tr.flat_grad.fill_(value)
        with Tape() as tape:
            loss = torch.zeros(1)
            record([], [loss], backward)
        tr._backward_and_update(tape, loss)
        assert tr._micro == (j + 1) % A
    assert log == EXPECTED[A, exchange, noisy], log
    assert tr._micro == 0 and not tr._noisy and tr.adam_step == 1
    # the first Adam step moves every parameter by lr * g / (|g| + eps / sqrt(1 - b2)) from the clean values: lr * sign(g)
    # up to eps / (sqrt(0.001) * |g|) <= 1.3e-6 of it at |g| >= 0.25
    torch.testing.assert_close(tr.flat, before - tr.last_lr, rtol=0, atol=2e-6 * tr.last_lr)
