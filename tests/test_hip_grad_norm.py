"""GPU tests of global-norm gradient clipping (clip_gradient_norm): nabu_grad_norm_f32 against float64 (1 ulp of fp32),
its factor and skip counter, nabu_adam_scaled_step against the clipping entry points it must equal bit for bit, the skip
on the device, argument errors, the trainer's trajectory against the float64 oracle with tests/grad_norm_ref.py, a
non-finite batch with and without weight noise, and two ranks on one GPU against one replica that accumulates."""
import math
import os

import numpy as np
import pytest
import torch

from nabu_amd import _hip
from nabu_amd import ops as hip
from nabu_amd.neuralnetworks.components import ops as nops
from tests import grad_norm_ref as R
from tests.test_grad_accum import batch_index
from tests.test_hip_grad_accum import CFG2, cfg2_data, make_trainer, params, ready, dev, bits, gradient
from tests.test_hip_model import encoder_layers, oracle_ctc_step, flat_oracle

pytestmark = pytest.mark.gpu

KEY = 'trainer.clip_gradient_norm'
ACCUM = 'trainer.numbatches_to_aggregate'
# the sizes of tests/test_hip_grad_accum.py (below a 16-byte group, a tail of three, one group, less than a block, more
# than one sweep of the 2048 x 256 x 4 grid with a tail of one) and 262 144: the smallest n with 257 stage-1 blocks, at
# which thread 0 of stage 2 takes a second partial
SIZES = [1, 3, 4, 1023, 262144, 4194309]
ADAM = (0.9, 0.999, 1e-8)
INF = math.inf
SCALE = 1.0 / 3


@pytest.fixture(scope='module')
def gradients():
    """(n, seed) -> (host gradient, device copy), made once per module and only read"""
    cache = {}

    def get(n, seed):
        if (n, seed) not in cache:
            g = gradient(n, seed)
            cache[(n, seed)] = (g, dev(g))
        return cache[(n, seed)]
    return get


def words(stats):
    """(norm, factor, skipped, word 3, all four words) of a stats buffer"""
    w = stats.cpu().numpy()
    f = w.view(np.float32)
    return f[0], f[1], int(w[2]), int(w[3]), w.copy()


def norm_of(g, acc, scale, c, stats=None):
    n = g.numel()
    fresh, ws = hip.grad_norm_buffers(n, g.device)
    stats = fresh if stats is None else stats
    assert hip.grad_norm(g, acc, scale, c, stats, ws) is stats
    return stats


def within_one_ulp(got, ref64):
    return abs(np.float64(got) - ref64) <= np.spacing(np.float32(ref64))


# ---------------------------------------------------------------------------------------------------------- grad_norm

@pytest.mark.parametrize('with_acc', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_norm_is_within_one_ulp_and_the_factor_is_the_stated_expression(n, with_acc, gradients):
    g, gd = gradients(n, 0)
    a, ad = gradients(n, 1) if with_acc else (None, None)
    x = a + g if with_acc else g                                  # the fp32 sum the Adam launch forms
    assert x.dtype == np.float32
    ref = np.float64(np.float32(SCALE)) * R.global_norm(x)
    for c in (0.5 * ref, 2.0 * ref):
        st = norm_of(gd, ad, SCALE, c)
        norm, factor, skipped, w3, all4 = words(st)
        print('n %d acc %s c %.6g: norm %.9g, float64 %.17g, factor %.9g' % (n, with_acc, c, norm, ref, factor))
        assert within_one_ulp(norm, ref), (norm, ref)
        want = R.factor_f32(norm, SCALE, c)                       # from the device's own norm word
        assert bits(np.array([factor])) == bits(np.array([want])), (factor, want)
        if c > ref:
            assert factor == np.float32(SCALE)                    # not clipped: the scale exactly
        else:
            assert factor == pytest.approx(SCALE * 0.5, rel=1e-6)
        assert skipped == 0 and w3 == 0
        again = words(norm_of(gd, ad, SCALE, c))[4]
        np.testing.assert_array_equal(again, all4)                # two calls, the same bits
    np.testing.assert_array_equal(bits(gd), bits(g))              # g and acc were only read
    if with_acc:
        np.testing.assert_array_equal(bits(ad), bits(a))


def test_extreme_magnitudes():
    n = 1023
    big = torch.full((n,), 1e30, device='cuda')
    norm, factor, skipped, _, _ = words(norm_of(big, None, 1.0, 1.0))
    ref = np.float64(np.float32(1e30)) * math.sqrt(n)
    assert np.isfinite(norm) and within_one_ulp(norm, ref) and skipped == 0      # finite and clipped, not skipped
    assert factor == R.factor_f32(norm, 1.0, 1.0) and 0 < factor < 1e-30
    # ... and with an accumulator whose fp32 sum with g is still finite
    norm, _, skipped, _, _ = words(norm_of(big, big.clone(), 0.5, 1.0))
    assert within_one_ulp(norm, 0.5 * 2.0 * np.float64(np.float32(1e30)) * math.sqrt(n)) and skipped == 0
    small = torch.full((n,), 1e-30, device='cuda')
    norm, factor, skipped, _, _ = words(norm_of(small, None, 1.0, 1.0))
    ref = np.float64(np.float32(1e-30)) * math.sqrt(n)
    assert norm > 0 and within_one_ulp(norm, ref) and factor == 1.0 and skipped == 0
    zeros = torch.zeros(n, device='cuda')
    norm, factor, skipped, _, _ = words(norm_of(zeros, None, SCALE, 1.0))
    assert norm == 0.0 and factor == np.float32(SCALE) and skipped == 0          # no division, no NaN
    g = torch.zeros(n, device='cuda')
    g[0], g[1] = 3.0, 4.0
    norm, factor, skipped, _, _ = words(norm_of(g, None, 1.0, 5.0))
    assert norm == 5.0 and factor == 1.0 and skipped == 0                        # exactly at max_norm: not clipped


def test_a_non_finite_element_in_the_last_tail_gives_a_nan_factor_and_counts(gradients):
    n = SIZES[-1]
    g, gd = gradients(n, 0)
    stats, _ = hip.grad_norm_buffers(n, gd.device)
    assert words(stats)[2] == 0
    for k, bad in enumerate((float('nan'), float('inf'))):
        poisoned = gd.clone()
        poisoned[n - 1] = bad
        norm, factor, skipped, w3, _ = words(norm_of(poisoned, None, SCALE, 1.0, stats))
        assert (np.isnan(norm) if k == 0 else norm == np.inf), norm
        assert np.isnan(factor) and skipped == k + 1 and w3 == 0
    norm, factor, skipped, _, _ = words(norm_of(gd, None, SCALE, 1.0, stats))
    assert np.isfinite(norm) and np.isfinite(factor) and skipped == 2             # never cleared by the kernel


def test_grad_norm_argument_errors_are_returned():
    n = 4096
    buf = torch.zeros(2 * n + 8, device='cuda')
    g, acc = buf[:n], buf[n:2 * n]
    g.fill_(3.0)
    acc.fill_(1.0)
    ibuf = torch.full((12,), 7, dtype=torch.int32, device='cuda')
    stats = ibuf[4:8]
    _, ws = hip.grad_norm_buffers(n, 'cuda')
    ws.fill_(-1.0)
    assert ws.numel() == 5                                       # ceil((4096 / 4 + 1) / 256) partial sums
    before = [bits(buf).copy(), ibuf.cpu().numpy().copy(), ws.cpu().numpy().copy()]

    def fails(text, x=g, a=acc, scale=SCALE, c=1.0, st=stats, w=ws):
        with pytest.raises(_hip.NabuHipError, match=text):
            hip.grad_norm(x, a, scale, c, st, w)
    fails('aligned', x=buf[1:n + 1], a=None)
    fails('aligned', a=buf[n + 1:2 * n + 1])
    fails('aligned', st=ibuf[5:9])
    fails('aligned', w=torch.zeros(64, dtype=torch.uint8, device='cuda')[4:])
    fails('null pointer', st=None)
    fails('workspace', w=ws[:4])
    fails('workspace', w=None)
    for c in (0.0, -1.0, float('nan')):
        fails('max_norm', c=c)
    for scale in (0.0, -0.5, float('inf'), float('nan')):
        fails('scale', scale=scale)
    fails('overlap', a=buf[4:n + 4])
    fails('overlap', a=g)
    fails('elements', a=buf[n:2 * n + 4])
    fails('int32', st=torch.zeros(4, device='cuda'))
    torch.cuda.synchronize()
    for was, now in zip(before, (bits(buf), ibuf.cpu().numpy(), ws.cpu().numpy())):
        np.testing.assert_array_equal(now, was)                  # nothing was launched
    hip.grad_norm(g, acc, SCALE, 1.0, stats, ws)                  # and a good call still runs
    assert words(stats)[0] == np.float32(np.float64(np.float32(SCALE)) * 4.0 * 64.0) and ibuf[3] == 7 and ibuf[8] == 7
    # adam_scaled_step: the checks of adam_clip_step_acc, plus the stats pointer
    p, m, v = (torch.zeros(n, device='cuda') for _ in range(3))
    kept = bits(buf).copy()

    def step_fails(text, out=p, src=None, a=None, x=g, st=stats):
        with pytest.raises(_hip.NabuHipError, match=text):
            hip.adam_scaled_step(out, src, a, x, m, v, 1e-3, *ADAM, st)
    step_fails('aligned', x=buf[1:n + 1])
    step_fails('aligned', st=ibuf[5:9])
    step_fails('null pointer', st=None)
    step_fails('overlap', src=p)
    step_fails('overlap', a=g)
    step_fails('elements', a=buf[n:2 * n + 4])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(buf), kept)
    assert float(p.abs().max()) == 0 and float(m.abs().max()) == 0 and float(v.abs().max()) == 0


# --------------------------------------------------------------------------------------------------- adam_scaled_step

def state(n):
    rng = np.random.default_rng(n)
    return (dev(rng.normal(size=n).astype(np.float32)), dev((0.1 * rng.normal(size=n)).astype(np.float32)),
            dev((0.01 * rng.random(size=n)).astype(np.float32)))


@pytest.mark.parametrize('n', SIZES)
def test_scaled_step_is_the_parent_kernels_bit_for_bit(n, gradients):
    """the entry points from before this feature, called with clip = +inf and the factor the device produced"""
    p0, m0, v0 = state(n)
    _, gd = gradients(n, 0)
    _, ad = gradients(n, 1)
    lr_t = 2.5e-3
    for with_acc in (False, True):
        acc = ad if with_acc else None
        unclipped = words(norm_of(gd, acc, SCALE, 1e30))[0]
        for c in (0.5 * float(unclipped), 2.0 * float(unclipped)):
            stats = norm_of(gd, acc, SCALE, c)
            factor = float(words(stats)[1])
            assert (factor == np.float32(SCALE)) == (c > unclipped) and factor > 0
            for with_src in (False, True):
                ref = [p0.clone(), m0.clone(), v0.clone()]
                src = p0 if with_src else None
                if with_acc:
                    if with_src:                                 # (also the two-launch form: accumulate, then _from)
                        total = hip.clip_accumulate(torch.empty_like(gd), ad, gd, INF)
                        two = [torch.empty_like(p0), m0.clone(), v0.clone()]
                        hip.adam_clip_step_from(two[0], p0, total, two[1], two[2], lr_t, *ADAM, INF, factor)
                    hip.adam_clip_step_acc(ref[0], src, ad, gd, ref[1], ref[2], lr_t, *ADAM, INF, factor)
                    if with_src:
                        assert all(torch.equal(x, y) for x, y in zip(two, ref))
                elif with_src:
                    hip.adam_clip_step_from(ref[0], p0, gd, ref[1], ref[2], lr_t, *ADAM, INF, factor)
                else:
                    hip.adam_clip_step(ref[0], gd, ref[1], ref[2], lr_t, *ADAM, INF, factor)
                got = [torch.full_like(p0, float('nan')) if with_src else p0.clone(), m0.clone(), v0.clone()]
                hip.adam_scaled_step(got[0], p0.clone() if with_src else None, acc, gd, got[1], got[2], lr_t, *ADAM, stats)
                for x, y in zip(got, ref):
                    assert torch.equal(x, y), (with_acc, with_src, c)
                assert not torch.equal(got[0], p0) and not torch.equal(got[1], m0)


@pytest.mark.parametrize('n', [3, 1023, SIZES[-1]])
def test_a_nan_factor_skips_the_update_on_the_device(n, gradients):
    p0, m0, v0 = state(n)
    _, gd = gradients(n, 0)
    _, ad = gradients(n, 1)
    poisoned = gd.clone()
    poisoned[n - 1] = float('nan')
    stats = norm_of(poisoned, None, SCALE, 1.0)
    assert np.isnan(words(stats)[1])
    for with_acc in (False, True):
        for with_src in (False, True):
            garbage = torch.full_like(p0, float('nan'))
            got = [garbage.clone() if with_src else p0.clone(), m0.clone(), v0.clone()]
            hip.adam_scaled_step(got[0], p0.clone() if with_src else None, ad if with_acc else None, poisoned, got[1],
                                 got[2], 2.5e-3, *ADAM, stats)
            for x, y in zip(got, (p0, m0, v0)):                  # m, v as they were; the parameter untouched, or = src
                np.testing.assert_array_equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------------- the trainer

def oracle_trajectory(data, A, updates, c, start):
    """`updates` updates of the float64 oracle with the restatement's rule; -> (losses, norms, layers)"""
    layers = [dict(l) for l in start[0]]
    W, bb = start[1], start[2]
    ms = [np.zeros_like(v) for v in flat_oracle(layers, W, bb)]
    vs = [np.zeros_like(v) for v in flat_oracle(layers, W, bb)]
    losses, norms = [], []
    for s in range(updates):
        micro = [oracle_ctc_step(data.batch(batch_index(s, j, 0, A, 1)), layers, W, bb, 'Listener') for j in range(A)]
        losses.append(np.mean([mb[0] for mb in micro]))
        per_batch = [flat_oracle(grads, dW, db) for _, grads, dW, db in micro]
        mean = [R.mean_gradient([g[i] for g in per_batch]) for i in range(len(per_batch[0]))]
        norm = R.global_norm(mean)
        norms.append(norm)
        f = c / norm if norm > c else 1.0
        new = []
        for i, p in enumerate(flat_oracle(layers, W, bb)):
            p2, ms[i], vs[i] = R.adam_update(p, mean[i] * f, ms[i], vs[i], s + 1, 1e-3)
            new.append(p2)
        for li, l in enumerate(layers):
            l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias'] = new[4 * li:4 * li + 4]
        W, bb = new[-2], new[-1]
    return losses, norms, layers


@pytest.mark.parametrize('A', [1, 2])
def test_cfg2_trajectory_matches_the_oracle(A):
    """4 updates of the shrunken cfg2 with the key set; bars of tests/test_hip_grad_accum.py::
    test_cfg2_trajectory_matches_the_oracle, the norm to the 2e-4 of test_single_step_gradients_match_oracle"""
    updates, nl = 4, 2
    data = cfg2_data()
    st = params(ready(make_trainer('cfg2_listener_ctc', data, CFG2)))
    start = (encoder_layers(st, 'Listener', nl), st['DNNDecoder/text/outlayer/weights'].astype(np.float64),
             st['DNNDecoder/text/outlayer/biases'].astype(np.float64))
    # c = half the smallest norm of the oracle's trajectory: an unclipped first pass finds the norms, the pass that
    # counts runs at the c they give and must itself stay above it
    _, norms, _ = oracle_trajectory(data, A, updates, INF, start)
    c = 0.5 * min(norms)
    ref_losses, norms, layers = oracle_trajectory(data, A, updates, c, start)
    print('A %d: c %.6g, oracle norms %s' % (A, c, norms))
    assert all(norm > c for norm in norms)                       # clipping is active at every update
    tr = make_trainer('cfg2_listener_ctc', data, CFG2, **{KEY: c, ACCUM: A})
    losses = []
    for s in range(updates):
        batches = [tr.to_device(data.batch(batch_index(s, j, 0, A, 1))) for j in range(A)]
        loss = tr.step(batches[0]) if A == 1 else tr.step_accumulated(batches)
        tr.global_step += 1
        losses.append(float(loss.item()))
        norm, factor, skipped = tr.grad_stats()
        print('update %d: norm %.9g (oracle %.9g), factor %.9g' % (s, norm, norms[s], factor))
        assert abs(norm - norms[s]) / norms[s] < 2e-4
        assert factor == pytest.approx(c / norm / A, rel=1e-6) and skipped == 0
        assert tr.last_lr == pytest.approx(1e-3, rel=1e-12)      # (cfg2 does not decay it: the oracle's constant)
    rel = np.abs(np.array(losses) - np.array(ref_losses)) / np.abs(ref_losses)
    print('losses', losses, 'oracle', ref_losses, 'rel', rel)
    assert rel.max() < 1e-3, (losses, ref_losses)
    assert rel.max() < 5e-5, (losses, ref_losses)
    got = encoder_layers(params(tr), 'Listener', nl)
    for a, b_ in zip(got, layers):
        for k in a:
            d = np.abs(a[k] - b_[k])
            print(k, 'max %.3e mean %.3e' % (d.max(), d.mean()))
            assert d.max() < 4.5e-3 and d.mean() < 2e-5, (k, d.max(), d.mean())
    assert tr.clip == INF and tr.clip_stats is not None


@pytest.mark.parametrize('noisy', [False, True])
def test_a_non_finite_batch_is_skipped_and_the_next_update_proceeds(noisy):
    data = cfg2_data()
    nops.set_seed(21)
    over = {KEY: 1.0}
    if noisy:
        over['trainer.weight_noise'] = 0.075
    tr = make_trainer('cfg2_listener_ctc', data, CFG2, **over)
    tr.step(tr.to_device(data.batch(0)))
    tr.global_step += 1
    assert tr.grad_stats()[2] == 0
    before = [tr.flat.clone(), tr.adam_m.clone(), tr.adam_v.clone()]
    inner, seen = tr._update, []

    def poisoned_update():
        seen.append(tr.flat.clone())                             # the parameters the step ran at
        tr.flat_grad[tr.flat_grad.numel() - 1] = float('nan')
        return inner()
    tr._update = poisoned_update
    loss = tr.step(tr.to_device(data.batch(1)))
    tr.global_step += 1
    tr._update = inner
    assert np.isfinite(float(loss.item())) and tr.adam_step == 2 and not tr._noisy
    assert torch.equal(seen[0], before[0]) != noisy              # with weight noise the step ran at other values
    for x, y in zip((tr.flat, tr.adam_m, tr.adam_v), before):
        np.testing.assert_array_equal(bits(x), bits(y))          # parameters (the clean ones), m and v: bit for bit
    norm, factor, skipped = tr.grad_stats()
    assert np.isnan(norm) and np.isnan(factor) and skipped == 1
    tr.step(tr.to_device(data.batch(2)))
    norm, factor, skipped = tr.grad_stats()
    assert np.isfinite(norm) and factor > 0 and skipped == 1 and tr.adam_step == 3
    assert not torch.equal(tr.flat, before[0]) and not torch.equal(tr.adam_m, before[1])
    assert bool(torch.isfinite(tr.flat).all())


def test_two_ranks_on_one_gpu_clip_to_identical_parameters(tmp_path):
    """two real ranks sharing the device, flat and bucketed exchange, 3 updates with the key set: the ranks end
    bit-identical, the two exchanges agree, and both equal — bit for bit — one replica that takes the same batches with
    numbatches_to_aggregate = 2: the all-reduce of two ranks and acc + g are the same single fp32 add per element, and
    the norm is reduced over the same values in the same order"""
    import socket
    import subprocess
    import sys
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'grad_norm_two_ranks.py')
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
    fields = ('flat', 'adam_m', 'adam_v', 'stats')
    for mode in ('flat', 'buckets'):
        for f in fields:
            name = mode + '/' + f
            np.testing.assert_array_equal(bits(a[name]), bits(b[name]), err_msg=name)             # rank 0 == rank 1
            np.testing.assert_array_equal(bits(a[name]), bits(a['single/' + f]), err_msg=name)    # == one replica, A = 2
        assert not np.array_equal(a[mode + '/losses'], b[mode + '/losses'])      # the ranks saw different batches
        assert np.isfinite(a[mode + '/losses']).all() and len(a[mode + '/losses']) == 3
        norms = a[mode + '/norms']
        assert len(norms) == 3 and (norms > float(a['c'])).all()                 # clipping was active at every update
    assert not np.array_equal(a['flat/flat'], a['initial'])
    assert int(a['single/stats'].view(np.int32)[2]) == 0
