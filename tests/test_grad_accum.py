"""CPU: gradient accumulation, the [trainer] key numbatches_to_aggregate = A * replicas.  The key's validation, the
batch schedule of both training loops on the stubbed trainer of tests/test_validation_loop.py, the update's arithmetic
(clip every micro-batch's gradient, sum, Adam on the mean) against the oracle with torch float64 stand-ins for the
kernels, two gloo ranks with the flat and the bucketed exchange, and the calls a trainer without the key makes."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import test_train_loop_overlap as overlap

KEY = 'trainer.numbatches_to_aggregate'


# ------------------------------------------------------------------------------------------------ float64 restatements

def mean_of_clipped(grads, clip=1.0):
    """the gradient an accumulated (or data-parallel) update applies: every gradient clipped on its own, then the mean"""
    return np.mean([np.clip(np.asarray(g, np.float64), -clip, clip) for g in grads], 0)


def batch_index(update, micro, rank, A, world):
    """the batch update `update`, micro-batch `micro`, rank `rank` reads: the sequence A * world replicas read"""
    return (update * A + micro) * world + rank


# ---------------------------------------------------------------------------------------------------- kernel stand-ins

def clip_(g, clip=1.0):
    g.clamp_(-clip, clip)
    return g


def adam(p, g, m, v, lr_t, b1, b2, eps, clip, gscale):
    x = (g * gscale).clamp(-clip, clip)
    m.mul_(b1).add_((1 - b1) * x)
    v.mul_(b2).add_((1 - b2) * x * x)
    p.sub_(lr_t * m / (v.sqrt() + eps))


def adam_from(p, src, g, m, v, lr_t, b1, b2, eps, clip, gscale):
    p.copy_(src)
    adam(p, g, m, v, lr_t, b1, b2, eps, clip, gscale)


def clip_accumulate(out, acc, g, clip=1.0):
    x = g.clamp(-clip, clip)
    out.copy_(x if acc is None else x + acc)
    return out


def adam_acc(p, src, acc, g, m, v, lr_t, b1, b2, eps, clip, gscale):
    if src is not None:
        p.copy_(src)
    adam(p, acc + g.clamp(-clip, clip), m, v, lr_t, b1, b2, eps, clip, gscale)


STAND_INS = dict(clip_=clip_, adam_clip_step=adam, adam_clip_step_from=adam_from, clip_accumulate=clip_accumulate,
                 adam_clip_step_acc=adam_acc)


def counted_stand_ins(monkeypatch):
    from nabu_amd import ops as hip
    counts = {}
    for name, fn in STAND_INS.items():
        def counted(*a, _fn=fn, _name=name, **k):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(hip, name, counted)
    return counts


class FakeServer(object):
    """what Trainer reads of a process group, for `world` replicas that all hold this process's gradient"""
    shared_devices = False

    def __init__(self, world):
        self.world_size, self.rank, self.reduced = world, 0, 0

    def all_reduce_sum_(self, t):
        self.reduced += 1
        return t.mul_(self.world_size)

    def broadcast_(self, t, src=0):
        return t


def make_trainer(server=None, **over):
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(2, 16, 40, seed=5, batches_per_epoch=10),
                                               modelconf=mc, evaluatorconf=ec, expdir=None, server=server, task_index=0)


def seed_optimizer(tr, theta0):
    n = len(theta0)
    tr.flat = torch.tensor(np.array(theta0, np.float64))
    tr.adam_m = torch.zeros(n, dtype=torch.float64)
    tr.adam_v = torch.zeros(n, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------ key validation

def test_key_values():
    from nabu_amd.neuralnetworks.trainers.trainer import aggregate_key
    assert aggregate_key({}, 1) == 1 and aggregate_key({}, 8) == 1                 # absent: the default 0
    for world in (1, 2, 8):
        assert aggregate_key({'numbatches_to_aggregate': '0'}, world) == 1
        assert aggregate_key({'numbatches_to_aggregate': str(world)}, world) == 1
        for A in (2, 3, 16):
            assert aggregate_key({'numbatches_to_aggregate': ' %d ' % (A * world)}, world) == A
    for text, world in (('-1', 1), ('-2', 2), ('2.5', 1), ('abc', 1), ('', 1), ('3', 2), ('1', 2), ('7', 8)):
        with pytest.raises(ValueError) as e:
            aggregate_key({'numbatches_to_aggregate': text}, world)
        msg = str(e.value)
        assert 'numbatches_to_aggregate' in msg and repr(text)[1:-1] in msg and '%d replica' % world in msg, msg
    with pytest.raises(ValueError, match='stale gradients'):
        aggregate_key({'numbatches_to_aggregate': '1'}, 2)


@pytest.mark.parametrize('value,world', [('-1', 1), ('2.5', 1), ('abc', 1), ('3', 2), ('1', 2)])
def test_a_bad_key_raises_in_the_constructor(value, world, monkeypatch):
    from nabu_amd.neuralnetworks.trainers import trainer as T
    built = []
    monkeypatch.setattr(T.Trainer, '_create_graph', lambda self: built.append(1))
    with pytest.raises(ValueError, match='numbatches_to_aggregate'):
        make_trainer(FakeServer(world) if world > 1 else None, **{KEY: value})
    assert not built                                                               # before any graph is built


def test_a_good_key_sets_the_micro_batch_count():
    assert make_trainer().accumulate == 1
    assert make_trainer(**{KEY: 0}).accumulate == 1 and make_trainer(**{KEY: 1}).accumulate == 1
    assert make_trainer(**{KEY: 3}).accumulate == 3
    assert make_trainer(FakeServer(2), **{KEY: 2}).accumulate == 1
    tr = make_trainer(FakeServer(2), **{KEY: 6})
    assert tr.accumulate == 3 and tr.flat_acc is None
    g = tr._create_graph()
    assert g['num_steps'] == 10 * int(tr.conf['num_epochs']) // 3
    with pytest.raises(ValueError, match='3 batches'):
        tr.step_accumulated([None, None])
    with pytest.raises(ValueError, match='call step'):
        make_trainer().step_accumulated([None])


# ------------------------------------------------------------------------------------------------------------ schedule

A = 3
SCRIPTS = {
    'plain': ([5.0, 4.0, 3.0, 2.0], dict(valid_frequency=4, num_tries='None')),
    'go_back': ([5.0, 6.0, 4.0, 4.5, 1.0, 0.9], dict(valid_frequency=3, num_tries='None', go_back='True',
                                                     valid_adapt='True')),
}


class StandardTrainer(overlap.StandardTrainer):
    """the stubbed trainer of the loop tests (fake step, scripted validation, logging batch source, identity stage), with
    the accumulated update stubbed the same way (same class name: the defaults file is looked up by it)"""

    def step_accumulated(self, batches):
        assert len(batches) == self.accumulate and self._micro == 0
        self.log.append(('update', self.global_step, [b['step'] for b in batches]))
        self.weights += 1.0
        self.last_lr = self.learning_rate()
        value = float(np.mean([10.0 - 0.01 * b['step'] for b in batches]))
        return overlap.LoggedLoss(value, self.global_step, self.log)

    def save_checkpoint(self, path):
        self.log.append(('checkpoint', self.global_step, self._micro))

    def save(self):
        pass


def run(script, prefetch, tmp_path=None, **over):
    over = dict(over, numbatches_to_aggregate=A, num_epochs=3, learning_rate_decay=0.5)
    if prefetch is not None:
        over['prefetch_batches'] = prefetch
    tr = StandardTrainer(script, **{'trainer.' + k: v for k, v in over.items()})
    if tmp_path is not None:
        tr.expdir, tr.checkpoint_steps = str(tmp_path), 2
    hist = tr.train()
    return tr, hist


@pytest.mark.parametrize('name', sorted(SCRIPTS))
def test_both_loops_read_the_batches_of_a_times_as_many_replicas(name, tmp_path):
    script, over = SCRIPTS[name]
    sync, hist = run(script, 0, tmp_path / 'sync', **over)
    ahead, hist2 = run(script, 2, tmp_path / 'ahead', **over)
    num_steps = 12 * 3 // A                                     # num_batches * num_epochs // A
    assert sync._graph['num_steps'] == ahead._graph['num_steps'] == num_steps
    updates = [e for e in sync.log if e[0] == 'update']
    assert len(hist) == len(updates)                            # one history entry per update
    assert [h[0] for h in hist] == [u[1] for u in updates]
    if name == 'plain':
        assert [u[1] for u in updates] == list(range(num_steps))
        assert [s for s, _ in sync.validation_history] == [0, 4, 8]
    else:
        # go-back at update 3 to update 0 and at update 6 to update 3: the indices resume at (s * A) * world
        assert [u[1] for u in updates] == [0, 1, 2, 0, 1, 2, 3, 4, 5, 3, 4, 5, 6, 7, 8, 9, 10, 11]
        assert [s for s, _ in sync.validation_history] == [0, 3, 3, 6, 6, 9]
    for _, s, idx in updates:
        assert idx == [batch_index(s, j, 0, A, 1) for j in range(A)], (s, idx)
    # the synchronous loop asks for exactly these batches, in this order: 0, 1, 2 | 3, 4, 5 | ...
    assert [e[1] for e in sync.log if e[0] == 'request'] == [i for u in updates for i in u[2]]
    if name == 'plain':
        assert [e[1] for e in sync.log if e[0] == 'request'][:6] == [0, 1, 2, 3, 4, 5]
    # the two loops: equal histories, equal batches per update, equal final state
    assert hist2 == hist
    assert [e for e in ahead.log if e[0] == 'update'] == updates
    assert ahead.validation_history == sync.validation_history
    assert (ahead.global_step, ahead.learning_rate_fact, ahead.weights, ahead.best_validation, ahead.num_tries) == \
        (sync.global_step, sync.learning_rate_fact, sync.weights, sync.best_validation, sync.num_tries)
    assert [e for e in ahead.log if e[0] == 'stage'] and all(not e[2] for e in ahead.log if e[0] == 'stage')
    # each loss is the mean over the update's batches, and the learning rate decays over updates
    for (s, loss, lr), u in zip(hist, updates):
        assert loss == pytest.approx(np.mean([10.0 - 0.01 * i for i in u[2]]), rel=1e-6)
    if name == 'plain':                                         # (no halving in between)
        lr0 = float(sync.conf['initial_learning_rate'])
        assert [lr for _, _, lr in hist] == pytest.approx([lr0 * 0.5 ** (s / num_steps) for s in range(num_steps)])
    # checkpoints (every 2 updates, and the final one) fall on update boundaries
    for tr in (sync, ahead):
        cps = [e for e in tr.log if e[0] == 'checkpoint']
        assert len(cps) >= num_steps // 2 and all(micro == 0 for _, _, micro in cps)
        assert cps[-1][1] == num_steps
        assert [e for e in cps] == [e for e in sync.log if e[0] == 'checkpoint']


def test_state_raises_in_the_middle_of_an_update(monkeypatch):
    counted_stand_ins(monkeypatch)
    tr = make_trainer(**{KEY: 2})
    tr._create_graph()
    seed_optimizer(tr, np.zeros(8))
    tr.flat_grad = torch.ones(8, dtype=torch.float64)
    tr._accumulate(0)
    with pytest.raises(Exception, match='middle of an update'):
        tr.state()
    with pytest.raises(Exception, match='cannot be accumulated'):
        tr._accumulate(1)                                       # the last micro-batch belongs to _update
    tr._update()
    assert tr._micro == 0 and tr.adam_step == 1


# ---------------------------------------------------------------------------------------------------- update arithmetic

def test_update_is_adam_on_the_mean_of_the_clipped_gradients(monkeypatch):
    from oracle import nabu_oracle as O
    counts = counted_stand_ins(monkeypatch)
    n = 1000
    rng = np.random.default_rng(7)
    theta0 = rng.normal(size=n)
    grads = [np.random.default_rng(100 + j).normal(0, 2, n) for j in range(A)]
    assert 0.55 < np.mean(np.abs(np.concatenate(grads)) > 1) < 0.68            # most elements are clipped
    tr = make_trainer(**{KEY: A})
    tr._create_graph()
    seed_optimizer(tr, theta0)
    m = np.zeros(n)
    v = np.zeros(n)
    theta = theta0
    for update in range(2):
        for j in range(A):
            tr.flat_grad = torch.tensor(grads[j] * (1 + update))
            if j < A - 1:
                tr._accumulate(j)
            else:
                tr._update()
        tr.global_step += 1
        lr = tr.last_lr
        ref, m2, v2 = O.clip_adam_update(theta, mean_of_clipped([g * (1 + update) for g in grads]), m, v, update + 1, lr)
        np.testing.assert_allclose(tr.flat.numpy(), ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(tr.adam_m.numpy(), m2, rtol=1e-12, atol=1e-14)
        if update == 0:
            wrong, _, _ = O.clip_adam_update(theta, np.mean(grads, 0), m, v, 1, lr)
            assert np.abs(wrong - ref).max() > 1e-6                              # clip(mean) is another update
        theta, m, v = ref, m2, v2
    assert counts == {'clip_accumulate': 2 * (A - 1), 'adam_clip_step_acc': 2}
    assert tr.adam_step == 2 and tr.flat_acc is not None and tr.flat_acc.numel() == n
    # the weight-noise form: the parameters come from the clean copy
    tr.flat_clean = torch.tensor(theta0.copy())
    tr.flat.fill_(1e9)
    tr._noisy = True
    for j in range(A):
        tr.flat_grad = torch.tensor(grads[j])
        tr._accumulate(j) if j < A - 1 else tr._update()
    ref, _, _ = O.clip_adam_update(theta0, mean_of_clipped(grads), m, v, 3, tr.last_lr)
    np.testing.assert_allclose(tr.flat.numpy(), ref, rtol=1e-12, atol=1e-14)
    assert not tr._noisy


def test_several_replicas_exchange_the_local_sum_once(monkeypatch):
    from oracle import nabu_oracle as O
    counts = counted_stand_ins(monkeypatch)
    n, world = 64, 2
    grads = [np.random.default_rng(j).normal(0, 2, n) for j in range(2)]
    server = FakeServer(world)
    tr = make_trainer(server, **{KEY: 2 * world})
    tr._create_graph()
    theta0 = np.linspace(-1, 1, n)
    seed_optimizer(tr, theta0)
    tr.flat_grad = torch.tensor(grads[0])
    tr._accumulate(0)
    tr.flat_grad = torch.tensor(grads[1])
    tr._update()
    # (FakeServer: both replicas hold the same two gradients)
    ref, _, _ = O.clip_adam_update(theta0, mean_of_clipped(grads + grads), np.zeros(n), np.zeros(n), 1, tr.last_lr)
    np.testing.assert_allclose(tr.flat.numpy(), ref, rtol=1e-12, atol=1e-14)
    assert server.reduced == 1 and counts == {'clip_accumulate': 2, 'adam_clip_step': 1}


# ------------------------------------------------------------------------------------------------------ unchanged calls

@pytest.mark.parametrize('world', [1, 2])
@pytest.mark.parametrize('key', [None, 0, 'world'])
def test_without_accumulation_the_update_makes_the_calls_it_always_made(key, world, monkeypatch):
    counts = counted_stand_ins(monkeypatch)
    over = {} if key is None else {KEY: world if key == 'world' else key}
    server = FakeServer(world) if world > 1 else None
    tr = make_trainer(server, **over)
    assert tr.accumulate == 1
    tr._create_graph()
    assert tr._graph['num_steps'] == 10 * int(tr.conf['num_epochs'])
    n = 32
    seed_optimizer(tr, np.zeros(n))
    tr.flat_grad = torch.tensor(np.random.default_rng(3).normal(0, 2, n))
    tr._update()
    plain = {'adam_clip_step': 1} if world == 1 else {'clip_': 1, 'adam_clip_step': 1}
    assert counts == plain
    counts.clear()
    tr.flat_clean, tr._noisy = tr.flat.clone(), True             # a weight-noise step
    tr._update()
    plain['adam_clip_step_from'] = plain.pop('adam_clip_step')
    assert counts == plain
    assert tr.flat_acc is None and tr._micro == 0 and tr.adam_step == 2


# ------------------------------------------------------------------------------------------------------ two gloo ranks

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    from oracle import nabu_oracle as O
    from nabu_amd import ops as hip
    from nabu_amd import recipes
    from nabu_amd.computing import dist
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    from tests.bench_standin import FakeModelStep

    server = dist.create_server(backend='gloo')
    for name, fn in STAND_INS.items():
        setattr(hip, name, fn)
    calls = []
    orig_sum, orig_async = server.all_reduce_sum_, server.all_reduce_sum_async

    def spy_sum(t):
        calls.append(('sum', int(t.numel())))
        return orig_sum(t)

    def spy_async(t):
        calls.append(('async', int(t.numel())))
        return orig_async(t)
    server.all_reduce_sum_, server.all_reduce_sum_async = spy_sum, spy_async

    # (1) the seam with synthetic gradients: K = 4 on two ranks, A = 2, four distinct gradients
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **{KEY: 4})
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(2, 16, 40, seed=5, batches_per_epoch=10),
                                             modelconf=mc, evaluatorconf=ec, expdir=None, server=server, task_index=rank)
    tr._create_graph()
    assert (tr.world, tr.accumulate) == (2, 2) and tr._graph['num_steps'] == 10 * int(tr.conf['num_epochs']) // 2
    n = 1000
    theta0 = np.random.default_rng(7).normal(size=n)
    grads = [np.random.default_rng(100 + i).normal(0, 2, n) for i in range(4)]      # grads[j * world + rank]
    seed_optimizer(tr, theta0)
    tr.flat_grad = torch.tensor(grads[batch_index(0, 0, rank, 2, world)].copy())
    tr._accumulate(0)
    assert not calls
    tr.flat_grad = torch.tensor(grads[batch_index(0, 1, rank, 2, world)].copy())
    tr._update()
    assert calls == [('sum', n)]                                   # exactly one all-reduce of the gradient per update
    ref, _, _ = O.clip_adam_update(theta0, mean_of_clipped(grads), np.zeros(n), np.zeros(n), 1, tr.learning_rate())
    np.testing.assert_allclose(tr.flat.numpy(), ref, rtol=1e-12, atol=1e-14)
    wrong, _, _ = O.clip_adam_update(theta0, np.mean(grads, 0), np.zeros(n), np.zeros(n), 1, tr.learning_rate())
    assert np.abs(wrong - ref).max() > 1e-6
    seam_sum = float(tr.flat.sum())

    # (2) flat against bucketed exchange through the fake model step: 2 updates of 2 micro-batches each
    finals = {}
    for mode in ('False', 'True'):
        del calls[:]
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **{'trainer.allreduce_buckets': mode, KEY: 4})
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(2, 16, 40), modelconf=mc,
                                                 evaluatorconf=ec, expdir=None, server=server, task_index=rank)
        fake = FakeModelStep(tr, server)
        for name, fn in STAND_INS.items():                         # (FakeModelStep installs its own two)
            setattr(hip, name, fn)
        numel = tr.flat_grad.numel()
        for update in range(2):
            fake.step()
            assert tr._micro == 1 and len(calls) == update * (4 if mode == 'True' else 1)
            fake.step()
            assert tr._micro == 0 and tr.adam_step == update + 1
        if mode == 'True':
            assert tr.buckets is not None and len(tr.buckets) == 4
            assert [c[0] for c in calls] == ['async'] * 8          # every bucket once per update
            assert sum(c[1] for c in calls) == 2 * numel
        else:
            assert calls == [('sum', numel)] * 2
        finals[mode] = tr.flat.clone()
    assert torch.equal(finals['False'], finals['True'])            # bit for bit
    assert float(finals['True'].abs().sum()) > 0
    q.put((rank, seam_sum, float(finals['True'].double().sum()), float(finals['False'].double().sum())))
    server.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_gloo_ranks_with_two_micro_batches_each():
    port = _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(150)
        assert p.exitcode == 0
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert res[0][1:] == res[1][1:]                                  # the ranks end identical
