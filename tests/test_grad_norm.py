"""CPU: global-norm gradient clipping, the [trainer] key clip_gradient_norm.  The key's validation, the ordered calls of
one update driven through Trainer._backward_and_update (the stand-ins and FakeServer of tests/test_grad_accum.py plus
float64 stand-ins for the two new wrappers), the update's arithmetic against tests/grad_norm_ref.py, the skip rule, and
that a trainer without the key neither calls the new wrappers nor allocates their buffers."""
import math

import numpy as np
import pytest
import torch

from tests import grad_norm_ref as R
from tests import test_grad_accum as accum
from tests.test_trainer_call_order import LoggingServer, N, BUCKETS, G, ACC, CLEAN, G0, G1, NOISE

KEY = 'trainer.clip_gradient_norm'
INF = math.inf


# ---------------------------------------------------------------------------------------------------- kernel stand-ins

def grad_norm(g, acc, scale, max_norm, stats, ws):
    """float64 stand-in of ops.grad_norm; `stats` is a float64 tensor of four values here"""
    x = (g if acc is None else acc + g).double()
    norm = float(scale) * math.sqrt(float((x * x).sum())) if bool(torch.isfinite(x).all()) else float('nan')
    finite = math.isfinite(norm)
    stats[0] = norm
    stats[1] = (scale * (max_norm / norm) if norm > max_norm else scale) if finite else float('nan')
    stats[2] += 0 if finite else 1
    stats[3] = 0
    return stats


def adam_scaled_step(p, src, acc, g, m, v, lr_t, b1, b2, eps, stats):
    factor = float(stats[1])
    if src is not None:
        p.copy_(src)
    if factor != factor:
        return
    x = (g if acc is None else acc + g) * factor
    m.mul_(b1).add_((1 - b1) * x)
    v.mul_(b2).add_((1 - b2) * x * x)
    p.sub_(lr_t * m / (v.sqrt() + eps))


def read_grad_stats(stats):
    return float(stats[0]), float(stats[1]), int(stats[2])


NEW = dict(grad_norm=grad_norm, adam_scaled_step=adam_scaled_step, read_grad_stats=read_grad_stats)


def counted_stand_ins(monkeypatch):
    from nabu_amd import ops as hip
    counts = accum.counted_stand_ins(monkeypatch)
    for name in ('grad_norm', 'adam_scaled_step'):
        def counted(*a, _fn=NEW[name], _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(hip, name, counted)
    monkeypatch.setattr(hip, 'read_grad_stats', read_grad_stats)
    return counts


def make_trainer(c, server=None, **over):
    tr = accum.make_trainer(server, **dict(over, **({} if c is None else {KEY: c})))
    tr._create_graph()
    return tr


def seed(tr, theta0):
    accum.seed_optimizer(tr, theta0)
    tr.clip_stats = torch.zeros(4, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------ key validation

def test_key_values():
    from nabu_amd.neuralnetworks.trainers.trainer import clip_norm_key
    assert clip_norm_key({}) == 0.0                                               # absent: off
    for text, value in (('0', 0.0), ('0.0', 0.0), (' 5 ', 5.0), ('1e-3', 1e-3), ('2.5', 2.5), ('1e30', 1e30)):
        assert clip_norm_key({'clip_gradient_norm': text}) == value
    for text in ('-1', '-0.5', 'nan', 'inf', '-inf', 'abc', '', 'None', '1,5'):
        with pytest.raises(ValueError) as e:
            clip_norm_key({'clip_gradient_norm': text})
        assert 'clip_gradient_norm' in str(e.value) and repr(text)[1:-1] in str(e.value), str(e.value)


@pytest.mark.parametrize('value', ['-1', 'nan', 'inf', 'abc'])
def test_a_bad_key_raises_in_the_constructor(value, monkeypatch):
    from nabu_amd.neuralnetworks.trainers import trainer as T
    built = []
    monkeypatch.setattr(T.Trainer, '_create_graph', lambda self: built.append(1))
    with pytest.raises(ValueError, match='clip_gradient_norm'):
        accum.make_trainer(None, **{KEY: value})
    assert not built                                                               # before any graph is built


def test_a_good_key_sets_the_mode():
    from nabu_amd.neuralnetworks.trainers.trainer import CLIP
    for tr in (accum.make_trainer(), accum.make_trainer(**{KEY: 0})):
        assert tr.clip_norm == 0.0 and tr.clip == CLIP == 1.0 and tr.clip_stats is None and tr.clip_ws is None
    tr = accum.make_trainer(accum.FakeServer(2), **{KEY: 2.5, accum.KEY: 6, 'trainer.weight_noise': 0.1})
    assert tr.clip_norm == 2.5 and tr.clip == INF and tr.accumulate == 3 and tr.clip_stats is None
    assert 'clip_gradient_norm' not in open(tr_defaults()).read()                  # an extension key


def tr_defaults():
    import os
    from nabu_amd.neuralnetworks.trainers import trainer as T
    return os.path.join(os.path.dirname(T.__file__), 'defaults', 'standardtrainer.cfg')


# ---------------------------------------------------------------------------------------------- the calls of one update

FIRST = ('clip_accumulate', ACC, None, G, INF)                 # (out, acc, g, clip)
NEXT = ('clip_accumulate', ACC, ACC, G, INF)
ACC0, ACC1 = 'flat_acc[0:8]', 'flat_acc[8:20]'


def expected(A, exchange, noisy):
    """the table of the feature's description: (buffer names; grad_norm: g, acc, scale; adam_scaled_step: src, acc)"""
    src = CLEAN if noisy else None
    calls = {
        (1, 'none'): [('grad_norm', G, None, 1.0), ('adam_scaled_step', src, None)],
        (1, 'flat'): [('all_reduce_sum_', G), ('grad_norm', G, None, 1 / 2), ('adam_scaled_step', src, None)],
        (1, 'bucketed'): [('all_reduce_sum_async', G0), ('all_reduce_sum_async', G1), ('grad_norm', G, None, 1 / 2),
                          ('adam_scaled_step', src, None)],
        (3, 'none'): [FIRST, NEXT, ('grad_norm', G, ACC, 1 / 3), ('adam_scaled_step', src, ACC)],
        (3, 'flat'): [FIRST, NEXT, ('clip_accumulate', G, ACC, G, INF), ('all_reduce_sum_', G),
                      ('grad_norm', G, None, 1 / 6), ('adam_scaled_step', src, None)],
        (3, 'bucketed'): [FIRST, NEXT, ('clip_accumulate', G0, ACC0, G0, INF), ('all_reduce_sum_async', G0),
                          ('clip_accumulate', G1, ACC1, G1, INF), ('all_reduce_sum_async', G1),
                          ('grad_norm', G, None, 1 / 6), ('adam_scaled_step', src, None)],
    }[A, exchange]
    return ([NOISE] if noisy else []) + calls


def logged_stand_ins(monkeypatch, log, name):
    """every wrapper the update path may call, logging its buffers first; the wrappers of the element-clipping mode are
    logged too, so that a call of one of them shows up in the list"""
    from nabu_amd import ops as hip
    S = dict(accum.STAND_INS, **NEW)
    entries = {
        'clip_': lambda g, clip=1.0: ('clip_', name(g)),
        'clip_accumulate': lambda out, acc, g, clip=1.0: ('clip_accumulate', name(out), name(acc), name(g), clip),
        'adam_clip_step': lambda p, g, *a: ('adam_clip_step', a[-1]),
        'adam_clip_step_from': lambda p, src, g, *a: ('adam_clip_step_from', name(src), a[-1]),
        'adam_clip_step_acc': lambda p, src, acc, g, *a: ('adam_clip_step_acc', name(src), name(acc), name(g), a[-1]),
        'grad_norm': lambda g, acc, scale, max_norm, stats, ws: ('grad_norm', name(g), name(acc), scale),
        'adam_scaled_step': lambda p, src, acc, g, *a: ('adam_scaled_step', name(src), name(acc)),
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
    monkeypatch.setattr(hip, 'set_phase_hook', lambda fn: None)
    monkeypatch.setattr(hip, 'read_grad_stats', read_grad_stats)


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
    c = 0.5                                                       # every update below has a larger norm: all are clipped
    over = {accum.KEY: A * world}
    if noisy:
        over['trainer.weight_noise'] = 0.125
    tr = make_trainer(c, LoggingServer(world, log, name) if world > 1 else None, **over)
    assert (tr.accumulate, tr.world, tr.clip_norm) == (A, world, c)
    seed(tr, torch.linspace(-1, 1, N, dtype=torch.float64).numpy())
    tr.flat_grad = torch.zeros(N, dtype=torch.float64)
    if exchange == 'bucketed':
        tr.buckets = [dict(key='b%d' % i, start=lo, end=hi, vars=[object()]) for i, (lo, hi) in enumerate(BUCKETS)]
    if noisy:
        from nabu_amd.neuralnetworks.components import ops as nops
        monkeypatch.setattr(nops.global_rng(), 'offset', nops.global_rng().offset)
        tr.flat_clean, tr.noise_table = torch.empty_like(tr.flat), None
        tr._add_weight_noise(None)
        assert tr._noisy
    before = tr.flat_clean.clone() if noisy else tr.flat.clone()
    values = [0.25 * (j + 1) for j in range(A)]
    for j in range(A):
        def backward(gout, value=values[j]):
            tr.flat_grad.fill_(value)
        with Tape() as tape:
            loss = torch.zeros(1)
            record([], [loss], backward)
        tr._backward_and_update(tape, loss)
        assert tr._micro == (j + 1) % A
    want = expected(A, exchange, noisy)
    assert len(log) == len(want), log
    for got, exp in zip(log, want):
        if got[0] == 'grad_norm':
            assert got[:3] == exp[:3] and got[3] == pytest.approx(exp[3], rel=1e-15), (got, exp)
        else:
            assert got == exp, (log, want)
    assert tr._micro == 0 and not tr._noisy and tr.adam_step == 1
    # the mean gradient is the constant mean(values): its norm is mean * sqrt(N) > c, so the factor is scale * c / norm
    mean = float(np.mean(values))
    norm, factor, skipped = tr.grad_stats()
    assert norm == pytest.approx(mean * math.sqrt(N), rel=1e-12) and norm > c and skipped == 0
    assert factor == pytest.approx(c / norm / (A * world), rel=1e-12)
    ref, _, _, _ = R.update(before.numpy(), [np.full(N, v) for v in values], np.zeros(N), np.zeros(N), 1, tr.last_lr, c)
    np.testing.assert_allclose(tr.flat.numpy(), ref, rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------------- update arithmetic

@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('A', [1, 3])
def test_five_updates_are_adam_on_the_norm_clipped_mean(A, world, monkeypatch):
    counts = counted_stand_ins(monkeypatch)
    n = 1000
    theta0 = np.random.default_rng(7).normal(size=n)
    base = [np.random.default_rng(100 + j).normal(0, 2, n) for j in range(A)]
    assert np.mean(np.abs(np.concatenate(base)) > 1) > 0.55        # the element clip would have changed most of them
    c = 1.5 * R.global_norm(R.mean_gradient(base))
    sizes = [0.5, 1.0, 2.0, 4.0, 8.0]                              # updates 0, 1 stay below c, updates 2..4 are clipped
    server = accum.FakeServer(world) if world > 1 else None
    tr = make_trainer(c, server, **{accum.KEY: A * world})
    seed(tr, theta0)
    theta, m, v = theta0, np.zeros(n), np.zeros(n)
    for u, size in enumerate(sizes):
        grads = [g * size for g in base]
        for j in range(A):
            tr.flat_grad = torch.tensor(grads[j].copy())
            if j < A - 1:
                tr._accumulate(j)
            else:
                tr._update()
        tr.global_step += 1
        # (FakeServer: every replica holds the same A gradients, the mean over A * world is the mean over A)
        theta, m, v, norm = R.update(theta, grads * world, m, v, u + 1, tr.last_lr, c)
        np.testing.assert_allclose(tr.flat.numpy(), theta, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(tr.adam_m.numpy(), m, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(tr.adam_v.numpy(), v, rtol=1e-12, atol=1e-14)
        got_norm, factor, skipped = tr.grad_stats()
        assert got_norm == pytest.approx(norm, rel=1e-12) and skipped == 0
        assert (norm > c) == (u >= 2)
        assert factor == pytest.approx(min(1.0, c / norm) / (A * world), rel=1e-12)
    want = {'grad_norm': 5, 'adam_scaled_step': 5}
    if A > 1:
        want['clip_accumulate'] = 5 * (A - 1 + (world > 1))
    assert counts == want
    assert (server.reduced if server else 0) == (5 if world > 1 else 0)


# ------------------------------------------------------------------------------------------------------------ the skip

@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('noisy', [False, True])
@pytest.mark.parametrize('A', [1, 2])
def test_a_non_finite_norm_skips_the_update(A, noisy, bad, monkeypatch):
    counted_stand_ins(monkeypatch)
    n, c = 64, 1.0
    rng = np.random.default_rng(3)
    theta0 = rng.normal(size=n)
    tr = make_trainer(c, **{accum.KEY: A})
    seed(tr, theta0)

    def run(grads, clean=None):
        if clean is not None:                                     # a weight-noise step: flat holds noisy values
            tr.flat_clean = torch.tensor(clean.copy())
            tr.flat.add_(0.3)
            tr._noisy = True
        for j, g in enumerate(grads):
            tr.flat_grad = torch.tensor(g.copy())
            tr._accumulate(j) if j < A - 1 else tr._update()
        tr.global_step += 1
        assert not tr._noisy

    good = [rng.normal(0, 2, n) for _ in range(A)]
    run(good)
    theta, m, v, _ = R.update(theta0, good, np.zeros(n), np.zeros(n), 1, tr.last_lr, c)
    np.testing.assert_allclose(tr.flat.numpy(), theta, rtol=1e-12, atol=1e-14)
    poisoned = [g.copy() for g in good]
    poisoned[0][n - 1] = bad                                      # with A = 2: in the accumulated sum, not in flat_grad
    kept = [tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone()]
    run(poisoned, clean=kept[0].numpy() if noisy else None)
    assert tr.adam_step == 2                                      # the host counts the skipped update
    assert torch.equal(tr.flat, kept[0]) and torch.equal(tr.adam_m, kept[1]) and torch.equal(tr.adam_v, kept[2])
    norm, factor, skipped = tr.grad_stats()
    assert not math.isfinite(norm) and factor != factor and skipped == 1
    theta2, m2, v2, _ = R.update(theta, poisoned, m, v, 2, tr.last_lr, c, clean=theta if noisy else None)
    assert np.array_equal(theta2, theta) and m2 is m and v2 is v  # the restatement skips as well
    run(good)                                                     # the next clean update proceeds, at t = 3
    theta3, m3, v3, _ = R.update(theta, good, m, v, 3, tr.last_lr, c)
    np.testing.assert_allclose(tr.flat.numpy(), theta3, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(tr.adam_m.numpy(), m3, rtol=1e-12, atol=1e-14)
    assert tr.grad_stats()[2] == 1 and math.isfinite(tr.grad_stats()[0])


def test_train_reports_skipped_updates_when_the_counter_moved(monkeypatch, capsys):
    counted_stand_ins(monkeypatch)
    tr = make_trainer(1.0)
    tr.task_index = 3
    tr._report_skipped()                                          # no buffer yet: nothing to read, nothing printed
    tr.clip_stats = torch.zeros(4, dtype=torch.float64)
    tr._report_skipped()
    assert capsys.readouterr().out == ''
    tr.clip_stats[2] = 2
    tr._report_skipped()
    tr._report_skipped()                                          # (the counter did not move again)
    assert capsys.readouterr().out == 'WORKER 3: 2 updates skipped (non-finite gradient norm)\n'
    assert 'clip_stats' not in tr.__class__.state.__code__.co_names         # nothing of it goes into state()


# ----------------------------------------------------------------------------------------------------- without the key

@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('A', [1, 3])
def test_without_the_key_nothing_new_is_called_or_allocated(A, world, monkeypatch):
    from nabu_amd import ops as hip
    counts = counted_stand_ins(monkeypatch)
    allocated = []
    monkeypatch.setattr(hip, 'grad_norm_buffers', lambda n, device: allocated.append(n) or (torch.zeros(4), None))
    server = accum.FakeServer(world) if world > 1 else None
    for c in (None, 0):
        tr = make_trainer(c, server, **{accum.KEY: A * world})
        tr.model.store.device = torch.device('cpu')               # (no variables yet: a flat buffer of one empty group)
        tr._init_optimizer()
        assert tr.clip_stats is None and tr.clip_ws is None and not allocated
        accum.seed_optimizer(tr, np.zeros(32))
        for j in range(A):
            tr.flat_grad = torch.tensor(np.random.default_rng(j).normal(0, 2, 32))
            tr._accumulate(j) if j < A - 1 else tr._update()
        with pytest.raises(Exception, match='clip_gradient_norm'):
            tr.grad_stats()
    assert 'grad_norm' not in counts and 'adam_scaled_step' not in counts and counts
    tr = make_trainer(5.0, server, **{accum.KEY: A * world})      # and with the key both buffers come from one call
    tr.model.store.device = torch.device('cpu')
    tr._init_optimizer()
    assert allocated == [tr.flat_grad.numel()] and tr.clip_stats is not None
