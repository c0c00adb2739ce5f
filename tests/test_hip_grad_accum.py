"""GPU tests of gradient accumulation (numbatches_to_aggregate = A * replicas): nabu_clip_accumulate_f32 against NumPy
float32, nabu_adam_clip_step_acc against the kernels it replaces (bit for bit) and against the float64 oracle, the
trainer's seam on the device, accumulated trajectories of a CTC and a cross-entropy recipe against the oracle and
against plain gradients combined on the host, Trainer.train with both loops, weight noise, and two ranks on one GPU."""
import os

import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from nabu_amd import _hip
from nabu_amd import ops as hip
from nabu_amd import recipes
from nabu_amd.autodiff import Tape
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.trainers import trainer_factory
from nabu_amd.processing.synthetic import SyntheticData
from tests.test_grad_accum import KEY, mean_of_clipped, batch_index
from tests.test_hip_model import encoder_layers, oracle_ctc_step, flat_oracle
from tests.test_hip_weight_noise import CFG3

pytestmark = pytest.mark.gpu

# 4 194 309 elements: more than one sweep of the 2048 x 256 x 4 grid (2 097 152), and a tail of one element
SIZES = [1, 3, 4, 1023, 4194309]
CLIP = 1.0
ADAM = (0.9, 0.999, 1e-8, CLIP)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def gradient(n, seed):
    """N(0, 2) in float32 (62 % beyond the clip), with elements exactly at +-clip and +-0 where they fit"""
    g = np.random.default_rng([n, seed]).normal(0, 2, n).astype(np.float32)
    special = np.array([CLIP, -CLIP, 0.0, -0.0, np.nextafter(np.float32(CLIP), np.float32(2)),
                        np.nextafter(np.float32(-CLIP), np.float32(-2))], np.float32)
    k = min(n, len(special))
    g[:k] = np.roll(special, seed)[:k]
    return g


@pytest.fixture(scope='module')
def gradients():
    """(n, seed) -> host gradient, computed once per module"""
    cache = {}

    def get(n, seed):
        if (n, seed) not in cache:
            cache[(n, seed)] = gradient(n, seed)
        return cache[(n, seed)]
    return get


# --------------------------------------------------------------------------------------------------- clip_accumulate

@pytest.mark.parametrize('n', SIZES)
def test_clip_accumulate_is_exact(n, gradients):
    g, a = gradients(n, 0), gradients(n, 1)
    clipped = np.clip(g, np.float32(-CLIP), np.float32(CLIP))
    assert clipped.dtype == np.float32
    gd, ad = dev(g), dev(a)
    # acc = NULL: a pure write (the NaN the output held is gone, nothing but g was read)
    out = torch.full_like(gd, float('nan'))
    assert hip.clip_accumulate(out, None, gd, CLIP) is out
    np.testing.assert_array_equal(out.cpu().numpy(), clipped)
    np.testing.assert_array_equal(bits(out), bits(clipped))             # (-0 stays -0)
    # out = acc
    acc = ad.clone()
    hip.clip_accumulate(acc, acc, gd, CLIP)
    np.testing.assert_array_equal(acc.cpu().numpy(), clipped + a)
    # out = g
    gg = gd.clone()
    hip.clip_accumulate(gg, ad, gg, CLIP)
    np.testing.assert_array_equal(gg.cpu().numpy(), clipped + a)
    np.testing.assert_array_equal(bits(ad), bits(a))                    # the accumulator was only read
    # out a buffer of its own
    out = torch.full_like(gd, float('nan'))
    hip.clip_accumulate(out, ad, gd, CLIP)
    np.testing.assert_array_equal(out.cpu().numpy(), clipped + a)
    np.testing.assert_array_equal(bits(gd), bits(g))
    assert np.mean(np.abs(g) > CLIP) > 0.5 or n < 100


def test_clip_accumulate_keeps_nan_visible():
    g = dev(np.array([np.nan, 3.0, -3.0, 0.5, np.nan], np.float32))
    out = hip.clip_accumulate(torch.empty_like(g), None, g, CLIP).cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[4]) and list(out[1:4]) == [1.0, -1.0, 0.5]


def test_clip_accumulate_argument_errors_are_returned():
    n = 64
    buf = torch.zeros(3 * n + 8, device='cuda')
    out, acc, g = buf[:n], buf[n:2 * n], buf[2 * n:3 * n]
    g.fill_(3.0)
    before = bits(buf).copy()

    def fails(text, o=out, a=acc, x=g):
        with pytest.raises(_hip.NabuHipError, match=text):
            hip.clip_accumulate(o, a, x, CLIP)
    fails('16-byte', o=buf[1:n + 1])                                     # unaligned pointers
    fails('16-byte', a=buf[n + 1:2 * n + 1])
    fails('16-byte', x=buf[2 * n + 2:3 * n + 2])
    fails('null pointer', x=None)
    fails('null pointer', o=None)
    fails('shifted overlap', o=buf[4:n + 4], a=out)                      # neither acc nor disjoint from it
    fails('shifted overlap', o=buf[2 * n - 4:3 * n - 4])
    fails('elements', a=buf[n:2 * n + 4])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(buf), before)                     # nothing was launched
    hip.clip_accumulate(out, None, g, CLIP)                              # and a good call still runs
    assert float(out.min()) == float(out.max()) == 1.0
    with pytest.raises(_hip.NabuHipError, match='overlap'):
        hip.adam_clip_step_acc(out, out, acc, g, buf[:n].clone(), buf[:n].clone(), 1e-3)
    with pytest.raises(_hip.NabuHipError, match='overlap'):
        hip.adam_clip_step_acc(out, None, g, g, buf[:n].clone(), buf[:n].clone(), 1e-3)


# ------------------------------------------------------------------------------------------------- adam_clip_step_acc

def parent_sequence(param, src, grads, m, v, lr_t, scale):
    """what the kernels before this feature compute for one accumulated update: clip_ on each gradient, axpy_ with
    a = 1 in the order of the micro-batches, then adam_clip_step (or _from) on the sum; updates param, m, v"""
    total = None
    for g in grads:
        c = hip.clip_(g.clone(), CLIP)
        total = c if total is None else hip.axpy_(total, c, 1.0)
    if src is None:
        hip.adam_clip_step(param, total, m, v, lr_t, *ADAM, scale)
    else:
        hip.adam_clip_step_from(param, src, total, m, v, lr_t, *ADAM, scale)


def accumulated_sequence(param, src, grads, m, v, lr_t, scale, acc):
    for j, g in enumerate(grads[:-1]):
        hip.clip_accumulate(acc, acc if j else None, g, CLIP)
    hip.adam_clip_step_acc(param, src, acc, grads[-1], m, v, lr_t, *ADAM, scale)


@pytest.mark.parametrize('n', SIZES)
def test_adam_acc_is_the_parent_kernels_sequence_bit_for_bit(n, gradients):
    A = 3
    rng = np.random.default_rng(n)
    p0 = dev(rng.normal(size=n).astype(np.float32))
    m0 = dev((0.1 * rng.normal(size=n)).astype(np.float32))
    v0 = dev((0.01 * rng.random(size=n)).astype(np.float32))
    grads = [dev(gradients(n, j)) for j in range(A)]
    kept = [g.clone() for g in grads]
    lr_t, scale = 2.5e-3, 1.0 / A
    for with_src in (False, True):
        ref = [p0.clone(), m0.clone(), v0.clone()]
        parent_sequence(ref[0], p0 if with_src else None, grads, ref[1], ref[2], lr_t, scale)
        # the candidate's output buffer holds garbage when the parameter comes from src
        got = [torch.full_like(p0, float('nan')) if with_src else p0.clone(), m0.clone(), v0.clone()]
        acc = torch.full_like(p0, float('nan'))
        accumulated_sequence(got[0], p0.clone() if with_src else None, grads, got[1], got[2], lr_t, scale, acc)
        for a, b in zip(got, ref):
            assert torch.equal(a, b)
        assert not torch.equal(got[0], p0)
        for g, k in zip(grads, kept):
            assert torch.equal(g, k)                                     # the gradients were only read


def test_adam_acc_matches_the_oracle_over_updates():
    """5 updates of A = 3 gradients each against clip_adam_update in float64 on the mean of the clipped gradients: the
    bars of tests/test_hip_ops.py::test_adam_clip_matches_oracle_over_steps on the same kind of inputs"""
    A, n = 3, 10007
    rng = np.random.default_rng(11)
    th = rng.normal(size=n)
    m = np.zeros(n)
    v = np.zeros(n)
    p, md, vd = dev(th.astype(np.float32)), dev(m.astype(np.float32)), dev(v.astype(np.float32))
    acc = torch.empty_like(p)
    for t in range(1, 6):
        gs = [rng.normal(0, 1.5, n).astype(np.float32) for _ in range(A)]
        th, m, v = O.clip_adam_update(th, mean_of_clipped(gs), m, v, t, 1e-3)
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        accumulated_sequence(p, None, [dev(g) for g in gs], md, vd, lr_t, 1.0 / A, acc)
    dp, dm = np.abs(p.cpu().numpy() - th).max(), np.abs(md.cpu().numpy() - m).max()
    print('max |dparam| %.3e, max |dm| %.3e' % (dp, dm))
    assert dp < 1e-6
    assert dm < 1e-6


# ------------------------------------------------------------------------------------------------------- the trainer

CFG2 = {'encoder.num_units': 16, 'encoder.num_layers': 2, 'trainer.batch_size': 5}


def cfg2_data(batches=100):
    return SyntheticData(5, 45, 40, min_frames=30, min_labels=2, max_labels=5, time_reduction=4, seed=2234,
                         batches_per_epoch=batches)           # T = 45 is odd: the pyramid pads


def cfg3_data():
    return SyntheticData(4, 32, 40, num_labels=39, min_frames=20, min_labels=2, max_labels=5, eos=True, time_reduction=8,
                         seed=3234)


def make_trainer(recipe, data, base, **over):
    mc, tc, ec = recipes.load_recipe(recipe, **dict(base, **over))
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0)


def ready(tr):
    tr._create_graph()
    tr._ensure_variables()
    if tr.flat is None:
        tr._init_optimizer()
    return tr


def params(tr):
    torch.cuda.synchronize()
    return {k: v.copy() for k, v in tr.model.store.state_dict().items()}


def lr_t_of(tr, t):
    return tr.learning_rate() * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)


def forward_backward(tr, batch):
    """the loss and the gradient of one batch at the trainer's weights, without an update"""
    with Tape() as tape:
        logits, lsl = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'], batch['target_seq_length'],
                               True)
        loss = tr.loss_fn(batch['targets'], logits, lsl, batch['target_seq_length'])
    tape.backward(loss)
    return loss


def test_trainer_seam_on_the_device():
    A = 3
    tr = ready(make_trainer('cfg2_listener_ctc', cfg2_data(), CFG2, **{KEY: A}))
    n = tr.flat.numel()
    assert tr.accumulate == A and tr.flat_acc is None and n % 4 == 0
    grads = [dev(np.random.default_rng([n, j]).normal(0, 2, n).astype(np.float32)) for j in range(A)]
    ref = [tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone()]
    parent_sequence(ref[0], None, grads, ref[1], ref[2], lr_t_of(tr, 1), 1.0 / A)
    wrong = [tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone()]
    mean = (grads[0].double() + grads[1].double() + grads[2].double()).div(A).float()
    hip.adam_clip_step(wrong[0], mean, wrong[1], wrong[2], lr_t_of(tr, 1), *ADAM, 1.0)
    for j in range(A):
        tr.flat_grad.copy_(grads[j])
        if j < A - 1:
            tr._accumulate(j)
        else:
            tr._update()
    assert tr._micro == 0 and tr.adam_step == 1 and tr.flat_acc.numel() == n
    assert torch.equal(tr.flat, ref[0]) and torch.equal(tr.adam_m, ref[1]) and torch.equal(tr.adam_v, ref[2])
    assert float((tr.flat - wrong[0]).abs().max()) > 1e-6               # clip-after-mean is another update


def test_cfg2_trajectory_matches_the_oracle():
    """3 accumulated updates over 9 batches; the oracle clips each micro-batch's gradients, averages them and applies
    clip_adam_update.  Bars of tests/test_hip_model.py::test_training_trajectory_matches_oracle."""
    A, updates = 3, 3
    data = cfg2_data()
    tr = make_trainer('cfg2_listener_ctc', data, CFG2, **{KEY: A})
    losses = []
    for s in range(updates):
        loss = tr.step_accumulated([tr.to_device(data.batch(batch_index(s, j, 0, A, 1))) for j in range(A)])
        tr.global_step += 1
        losses.append(float(loss.item()))
    assert tr.adam_step == updates
    tr2 = ready(make_trainer('cfg2_listener_ctc', data, CFG2))
    st = params(tr2)
    nl = 2
    layers = encoder_layers(st, 'Listener', nl)
    W = st['DNNDecoder/text/outlayer/weights'].astype(np.float64)
    bb = st['DNNDecoder/text/outlayer/biases'].astype(np.float64)
    ms = [np.zeros_like(v) for v in flat_oracle(layers, W, bb)]
    vs_ = [np.zeros_like(v) for v in flat_oracle(layers, W, bb)]
    ref_losses = []
    for s in range(updates):
        micro = [oracle_ctc_step(data.batch(batch_index(s, j, 0, A, 1)), layers, W, bb, 'Listener') for j in range(A)]
        ref_losses.append(np.mean([mb[0] for mb in micro]))
        per_batch = [flat_oracle(grads, dW, db) for _, grads, dW, db in micro]
        new = []
        for i, p in enumerate(flat_oracle(layers, W, bb)):
            p2, ms[i], vs_[i] = O.clip_adam_update(p, mean_of_clipped([g[i] for g in per_batch]), ms[i], vs_[i], s + 1, 1e-3)
            new.append(p2)
        for li, l in enumerate(layers):
            l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias'] = new[4 * li:4 * li + 4]
        W, bb = new[-2], new[-1]
    rel = np.abs(np.array(losses) - np.array(ref_losses)) / np.abs(ref_losses)
    print('losses', losses, 'oracle', ref_losses, 'rel', rel)
    assert rel.max() < 1e-3, (losses, ref_losses)
    assert rel.max() < 5e-5, (losses, ref_losses)
    got = encoder_layers(params(tr), 'Listener', nl)
    for a, b_ in zip(got, layers):
        for k in a:
            d = np.abs(a[k] - b_[k])
            assert d.max() < 4.5e-3 and d.mean() < 2e-5, (k, d.max(), d.mean())


def test_cfg3_trajectory_matches_plain_gradients_combined_on_the_host():
    """the cross-entropy path: 3 accumulated updates of the shrunken cfg3 against a trainer without the key that only
    supplies each micro-batch's loss and gradient at the reference weights; clip, mean and Adam run on the host in
    float64.  Same bars as the CTC trajectory."""
    A, updates = 3, 3
    data = cfg3_data()
    tr = make_trainer('cfg3_las_vanilla', data, CFG3, **{KEY: A})
    losses, lrs = [], []
    for s in range(updates):
        loss = tr.step_accumulated([tr.to_device(data.batch(batch_index(s, j, 0, A, 1))) for j in range(A)])
        tr.global_step += 1
        losses.append(float(loss.item()))
        lrs.append(tr.last_lr)                     # (the schedule over updates is host arithmetic: tests/test_grad_accum.py)
    plain = ready(make_trainer('cfg3_las_vanilla', data, CFG3))
    assert plain.accumulate == 1 and plain.flat.numel() == tr.flat.numel()
    theta = plain.flat.cpu().numpy().astype(np.float64)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    ref_losses = []
    for s in range(updates):
        ls, gs = [], []
        for j in range(A):
            loss = forward_backward(plain, plain.to_device(data.batch(batch_index(s, j, 0, A, 1))))
            ls.append(float(loss.item()))
            gs.append(plain.flat_grad.cpu().numpy().astype(np.float64))
        ref_losses.append(np.mean(ls))
        theta, m, v = O.clip_adam_update(theta, mean_of_clipped(gs), m, v, s + 1, lrs[s])
        plain.flat.copy_(torch.from_numpy(theta.astype(np.float32)))
    rel = np.abs(np.array(losses) - np.array(ref_losses)) / np.abs(ref_losses)
    print('losses', losses, 'reference', ref_losses, 'rel', rel)
    assert rel.max() < 1e-3, (losses, ref_losses)
    assert rel.max() < 5e-5, (losses, ref_losses)
    got, want = params(tr), params(plain)
    moved = 0
    for k in got:
        d = np.abs(got[k].astype(np.float64) - want[k])
        assert d.max() < 4.5e-3 and d.mean() < 2e-5, (k, d.max(), d.mean())
        moved += int(d.max() < 4.5e-3)
    assert moved == len(got) > 0
    assert np.abs(tr.flat.cpu().numpy() - ready(make_trainer('cfg3_las_vanilla', data, CFG3)).flat.cpu().numpy()).max() > 1e-4


def test_train_with_two_micro_batches_in_both_loops():
    A, updates = 2, 4
    over = dict(CFG2, **{KEY: A, 'trainer.num_epochs': 1, 'evaluator.evaluator': 'None'})

    def run(prefetch):
        tr = make_trainer('cfg2_listener_ctc', cfg2_data(batches=A * updates), over,
                          **({'trainer.prefetch_batches': prefetch} if prefetch else {}))
        return tr, tr.train()
    sync, hist = run(0)
    ahead, hist2 = run(2)
    assert [h[0] for h in hist] == list(range(updates)) and hist2 == hist
    want, got = params(sync), params(ahead)
    for k in want:
        np.testing.assert_array_equal(bits(want[k]), bits(got[k]), err_msg=k)
    # every loss is the mean of its two micro-batch losses, recomputed by a trainer without the key at the same weights
    data = cfg2_data(batches=A * updates)
    again = make_trainer('cfg2_listener_ctc', data, over)
    fresh = ready(make_trainer('cfg2_listener_ctc', data, dict(CFG2, **{'evaluator.evaluator': 'None'})))
    assert fresh.accumulate == 1
    again._create_graph()
    for s in range(updates):
        batches = [data.batch(batch_index(s, j, 0, A, 1)) for j in range(A)]
        if s:
            fresh.flat.copy_(again.flat)
        micro = [np.float32(forward_backward(fresh, fresh.to_device(b)).item()) for b in batches]
        loss = float(again.step_accumulated([again.to_device(b) for b in batches]).item())
        again.global_step += 1
        assert loss == float((micro[0] + micro[1]) * np.float32(0.5)), (s, loss, micro)
        assert loss == hist[s][1]


NOISE = {'trainer.weight_noise': 0.075}


def test_weight_noise_is_drawn_once_per_update(monkeypatch):
    A, updates = 3, 2
    counts = {}
    plain_clip, plain_adam_from = hip.clip_, hip.adam_clip_step_from    # for the test's own recomputation
    for fname in ('weight_noise', 'adam_clip_step', 'adam_clip_step_from', 'adam_clip_step_acc', 'clip_accumulate', 'clip_'):
        def counted(*a, _fn=getattr(hip, fname), _name=fname, **k):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(hip, fname, counted)
    data = cfg2_data()
    nops.set_seed(21)
    tr = make_trainer('cfg2_listener_ctc', data, CFG2, **dict(NOISE, **{KEY: A}))
    tr._create_graph()
    seen = []
    inner = tr.loss_fn

    def watching(*a, **k):
        seen.append(tr.flat.clone())                                    # the parameters this micro-batch ran at
        return inner(*a, **k)
    tr.loss_fn = watching
    for s in range(updates):
        before = None if tr.flat is None else (tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone())
        offset = nops.global_rng().offset
        tr.step_accumulated([tr.to_device(data.batch(batch_index(s, j, 0, A, 1))) for j in range(A)])
        tr.global_step += 1
        assert nops.global_rng().offset == offset + 1                   # one offset per update (cfg2 draws nothing else)
        assert tr.last_weight_noise == (21, offset + 1) and not tr._noisy and tr._micro == 0
        mine = seen[-A:]
        assert all(torch.equal(mine[0], x) for x in mine[1:])           # all micro-batches saw the same noisy weights
        assert not torch.equal(mine[0], tr.flat_clean)
        if before is not None:
            # between updates flat holds the clean parameters: the update started from them, not from the noisy ones
            assert torch.equal(tr.flat_clean, before[0])
            total = plain_clip(tr.flat_grad.clone(), CLIP)
            hip.axpy_(total, tr.flat_acc, 1.0)
            out = torch.empty_like(tr.flat)
            assert tr.learning_rate() == tr.last_lr                     # (cfg2 does not decay it)
            plain_adam_from(out, before[0], total, before[1], before[2], lr_t_of(tr, s + 1), *ADAM, 1.0 / A)
            assert torch.equal(out, tr.flat)
    assert counts.get('weight_noise') == updates and counts.get('adam_clip_step_acc') == updates
    assert counts.get('clip_accumulate') == updates * (A - 1)
    assert counts.get('adam_clip_step_from', 0) == 0 and counts.get('adam_clip_step', 0) == 0 and counts.get('clip_', 0) == 0


def test_an_exception_in_a_micro_batch_restores_the_clean_parameters():
    A = 3
    data = cfg2_data()
    nops.set_seed(21)
    tr = make_trainer('cfg2_listener_ctc', data, CFG2, **dict(NOISE, **{KEY: A}))
    tr._create_graph()
    batches = [tr.to_device(data.batch(j)) for j in range(A)]
    tr.step_accumulated(batches)
    tr.global_step += 1
    before, m_before, step_before = params(tr), bits(tr.adam_m).copy(), tr.adam_step
    inner = tr.loss_fn
    state = {'calls': 0, 'noisy': None, 'micro': None}

    class Boom(Exception):
        pass

    def second_raises(*a, **k):
        state['calls'] += 1
        if state['calls'] == 2:                                         # micro-batch 1
            state['noisy'], state['micro'] = tr.flat.clone(), tr._micro
            raise Boom()
        return inner(*a, **k)
    tr.loss_fn = second_raises
    with pytest.raises(Boom):
        tr.step_accumulated(batches)
    assert state['micro'] == 1 and tr._micro == 0 and not tr._noisy
    assert not torch.equal(state['noisy'], tr.flat)                     # the noise had been applied
    after = params(tr)
    for k in before:
        np.testing.assert_array_equal(bits(before[k]), bits(after[k]), err_msg=k)
    np.testing.assert_array_equal(bits(tr.adam_m), m_before)
    assert tr.adam_step == step_before
    tr.state()                                                          # on an update boundary again
    loss = tr.step_accumulated(batches)                                 # the next update runs
    assert np.isfinite(float(loss.item())) and tr.adam_step == step_before + 1
    assert any(not np.array_equal(before[k], v) for k, v in params(tr).items())


def test_two_ranks_on_one_gpu_accumulate_to_identical_parameters(tmp_path):
    """two real ranks sharing the device (gloo group), numbatches_to_aggregate = 4: two micro-batches each per update,
    two updates with the flat and two with the bucketed exchange"""
    import socket
    import subprocess
    import sys
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'grad_accum_two_ranks.py')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, script, str(tmp_path)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = np.load(str(tmp_path / 'rank0.npz')), np.load(str(tmp_path / 'rank1.npz'))
    names = [n for n in a.files if not n.startswith('__')]
    assert names and set(a.files) == set(b.files)
    for n in names:
        np.testing.assert_array_equal(bits(a[n]), bits(b[n]), err_msg=n)            # the replicas end bit-identical
    flat = [n for n in names if n.startswith('flat/')]
    assert flat
    for n in flat:
        np.testing.assert_array_equal(bits(a[n]), bits(a['buckets/' + n[5:]]), err_msg=n)   # the two modes agree
        assert not np.array_equal(a[n], a['__initial/' + n[5:]]), n
    for mode in ('flat', 'buckets'):
        assert not np.array_equal(a['__losses_' + mode], b['__losses_' + mode])     # the ranks saw different batches
        assert np.isfinite(a['__losses_' + mode]).all() and len(a['__losses_' + mode]) == 2
        assert list(a['__exchanges_' + mode]) == list(b['__exchanges_' + mode])
    assert list(a['__exchanges_flat']) == [1, 1] and min(a['__exchanges_buckets']) > 1
