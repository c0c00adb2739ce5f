"""GPU tests of variational weight noise: nabu_weight_noise_f32 against the host Philox reference (oracle/philox.py),
nabu_adam_clip_step_from against nabu_adam_clip_step, and the [trainer] keys weight_noise / weight_noise_start_step
through Trainer.step and Trainer.train (one step against a hand-made noisy step, the start step, the key-less path, the
error path, resume, the overlapped loop, two ranks)."""
import os

import numpy as np
import pytest
import torch

from oracle import philox as P
from nabu_amd import _hip
from nabu_amd import ops as hip
from nabu_amd import recipes
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.trainers import trainer_factory
from nabu_amd.neuralnetworks.trainers.trainer import weight_noise_ranges
from nabu_amd.processing.synthetic import SyntheticData
from tests.test_weight_noise import STREAMS, N_LARGE, moment_bars

pytestmark = pytest.mark.gpu

# 3 000 004 elements are past grid_for's cap of 2048 blocks x 256 threads x 4 elements: the loop takes a second lap
SIZES = [4, 8, 4100, N_LARGE]
SIGMAS = [0.075, 1.0]
CAP = hip.WEIGHT_NOISE_MAX_RANGES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _noise_bound(z, rad, y, s):
    """|device - (x + s z)| allowed per element, z and y in float64 (tests/test_hip_regularisation.py, restated).
    Box-Muller on the device: ra = sqrtf(-2 logf(u1)) (u1 exact; logf <= 1 ulp, sqrtf <= 0.5 ulp: <= 1.5 ulp of ra),
    sincosf(fl(fl32(2 pi) u)) (<= 2 ulp of the result at the float32 angle), z = ra * cos (0.5 ulp): <= 4 ulp of |z|,
    doubled to 8 * 2^-24 |z|.  The angle itself: |fl32(2 pi) - 2 pi| u <= 1.75e-7 plus the product's rounding
    <= 2.4e-7 (half an ulp at 2 pi): 4.2e-7 rad, which moves z by up to ra * 4.2e-7 -- taken as ra * 5e-7.  Then
    y = fl(x + fl(s z)): 2^-24 s |z| + 2^-24 |y| (the kernel's fmaf rounds once, which only tightens this)."""
    e = 2.0 ** -24
    return s * (8 * e * np.abs(z) + 5e-7 * rad) + e * s * np.abs(z) + e * np.abs(y) + 1e-30


def tables(n):
    """name -> [first_group, end_group) pairs over the n / 4 groups"""
    g = n // 4
    t = {'empty': [], 'everything': [(0, g)], 'first': [(0, 1)], 'last': [(g - 1, g)],
         # single groups alternating with gaps (as many as the table takes: at the large size exactly the cap)
         'alternating': [(2 * k, 2 * k + 1) for k in range(min(CAP, (g + 1) // 2))]}
    if g >= 2:
        t['touching'] = [(0, g // 2), (g // 2, g)]       # two entries that meet
    return t


def group_mask(n, table):
    m = np.zeros(n // 4, bool)
    for a, b in table:
        m[a:b] = True
    return np.repeat(m, 4)


@pytest.fixture(scope='module')
def reference():
    """(n, stream) -> (z, radius) of the host Box-Muller, computed once per module"""
    cache = {}

    def get(n, stream):
        if (n, stream) not in cache:
            cache[(n, stream)] = P.gaussian(n, stream[0], stream[1], with_radius=True)
        return cache[(n, stream)]
    return get


# ------------------------------------------------------------------------------------------------- the noise kernel

@pytest.mark.parametrize('stream', STREAMS)
@pytest.mark.parametrize('n', SIZES)
def test_noise_kernel_against_the_host_reference(n, stream, reference):
    seed, offset = stream
    z, rad = reference(n, stream)
    x = np.random.default_rng(n).normal(size=n).astype(np.float32)
    xd = dev(x)
    for sigma in SIGMAS:
        s = float(np.float32(sigma))
        want = x.astype(np.float64) + s * z
        tol = _noise_bound(z, rad, want, s)
        whole = None
        for name, table in tables(n).items():
            param, clean = xd.clone(), torch.full_like(xd, -1234.5)
            out = hip.weight_noise(param, clean, hip.WeightNoiseTable(table, 'cuda'), sigma, seed, offset)
            assert out is param
            got = param.cpu().numpy()
            np.testing.assert_array_equal(bits(clean), bits(x), err_msg='clean, table %s' % name)
            inside = group_mask(n, table)
            np.testing.assert_array_equal(bits(got[~inside]), bits(x[~inside]), err_msg='outside, table %s' % name)
            err = np.abs(got.astype(np.float64) - want)[inside]
            if err.size:
                worst = int(err.argmax())
                assert np.all(err <= tol[inside]), (name, sigma, worst, err[worst], tol[inside][worst])
                assert (got[inside] != x[inside]).mean() > 0.9          # the noise is there
            if name == 'everything':
                whole = got
            elif whole is not None:
                # the values do not depend on the table: where two tables cover an element the bits agree
                np.testing.assert_array_equal(bits(got[inside]), bits(whole[inside]), err_msg='table %s' % name)
        if n == N_LARGE:
            d = (whole.astype(np.float64) - x.astype(np.float64)) / s
            mean_bar, std_bar = moment_bars(n)
            print('n %d stream %s sigma %g: mean %.3e (bar %.3e), std - 1 %.3e (bar %.3e)'
                  % (n, stream, sigma, d.mean(), mean_bar, d.std() - 1, std_bar))
            assert abs(d.mean()) <= mean_bar and abs(d.std() - 1.0) <= std_bar
    # stddev 0: an exact copy, in both buffers
    param, clean = xd.clone(), torch.empty_like(xd)
    hip.weight_noise(param, clean, hip.WeightNoiseTable(tables(n)['everything'], 'cuda'), 0.0, seed, offset)
    np.testing.assert_array_equal(bits(param), bits(x))
    np.testing.assert_array_equal(bits(clean), bits(x))


def test_noise_kernel_draws_what_gaussian_noise_draws():
    """the shared device function: weight noise over everything and input noise of the same array at the same stream
    are the same values up to the one rounding the fused multiply-add saves"""
    n = 4100
    x = dev(np.random.default_rng(5).normal(size=n).astype(np.float32))
    for seed, offset in STREAMS:
        y = hip.gaussian_noise(x, 0.6, seed, offset).cpu().numpy().astype(np.float64)
        param, clean = x.clone(), torch.empty_like(x)
        hip.weight_noise(param, clean, hip.WeightNoiseTable([(0, n // 4)], 'cuda'), 0.6, seed, offset)
        w = param.cpu().numpy().astype(np.float64)
        # both are roundings of x + fl32(0.6) z for ONE z: apart by at most an ulp of the sum plus half an ulp of 0.6 z
        assert np.all(np.abs(w - y) <= 2.0 ** -23 * np.abs(y) + 2.0 ** -24 * np.abs(y - clean.cpu().numpy()) + 1e-30)
        assert np.abs(w - clean.cpu().numpy()).max() > 0.1


def test_noise_kernel_argument_errors_are_returned():
    n = 64
    buf = torch.zeros(2 * n + 8, device='cuda')
    param, clean = buf[:n], buf[n:2 * n]
    before = bits(buf).copy()
    ok = [(0, 4), (4, 16)]

    def fails(text, p=param, c=clean, table=ok, sigma=0.075):
        with pytest.raises(_hip.NabuHipError, match=text):
            hip.weight_noise(p, c, hip.WeightNoiseTable(table, 'cuda'), sigma, 7, 3)
    fails('16-byte', p=buf[1:n + 1])                                     # unaligned pointers
    fails('16-byte', c=buf[n + 2:2 * n + 2])
    fails('overlap', c=buf[4:n + 4])
    fails('multiple of 4', p=buf[:62], c=buf[n:n + 62])                  # n % 4 != 0
    fails('unsorted', table=[(4, 16), (0, 4)])                           # unsorted
    fails('overlaps', table=[(0, 5), (4, 16)])                           # overlapping
    fails('past', table=[(0, 4), (4, 17)])                               # past the buffer
    fails('stddev', sigma=-1.0)
    fails('stddev', sigma=float('nan'))
    with pytest.raises(_hip.NabuHipError, match='elements'):
        hip.weight_noise(param, buf[n:2 * n + 4], hip.WeightNoiseTable(ok, 'cuda'), 0.075, 7, 3)
    big = torch.zeros(8 * (CAP + 1), device='cuda')                      # one range more than the cap
    with pytest.raises(_hip.NabuHipError, match='nranges = %d' % (CAP + 1)):
        hip.weight_noise(big, torch.empty_like(big), hip.WeightNoiseTable([(2 * k, 2 * k + 1) for k in range(CAP + 1)], 'cuda'),
                         0.075, 7, 3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(buf), before)                     # nothing was launched
    assert float(big.abs().max()) == 0.0
    hip.weight_noise(param, clean, hip.WeightNoiseTable(ok, 'cuda'), 0.075, 7, 3)      # and the good call still runs
    assert float(param.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- the optimiser

@pytest.mark.parametrize('n', [1, 5, 4099, 3000004])
def test_adam_from_is_adam_on_a_copy_of_the_source(n):
    rng = np.random.default_rng(n)
    src = dev(rng.normal(size=n).astype(np.float32))
    g = dev((3.0 * rng.normal(size=n)).astype(np.float32))              # some beyond the clip
    m0 = dev((0.1 * rng.normal(size=n)).astype(np.float32))
    v0 = dev((0.01 * rng.random(size=n)).astype(np.float32))
    args = (2.5e-3, 0.9, 0.999, 1e-8, 1.0, 0.5)
    p_ref, m_ref, v_ref = src.clone(), m0.clone(), v0.clone()
    hip.adam_clip_step(p_ref, g, m_ref, v_ref, *args)
    kept = src.clone()
    # param_out holds garbage the call must not read, and aliases nothing
    out, m, v = torch.full_like(src, float('nan')), m0.clone(), v0.clone()
    hip.adam_clip_step_from(out, src, g, m, v, *args)
    np.testing.assert_array_equal(bits(out), bits(p_ref))
    np.testing.assert_array_equal(bits(m), bits(m_ref))
    np.testing.assert_array_equal(bits(v), bits(v_ref))
    np.testing.assert_array_equal(bits(src), bits(kept))
    assert not np.array_equal(bits(out), bits(src))
    with pytest.raises(_hip.NabuHipError, match='overlap'):
        hip.adam_clip_step_from(src, src, g, m, v, *args)
    with pytest.raises(_hip.NabuHipError, match='elements'):
        hip.adam_clip_step_from(out, torch.zeros(n + 4, device='cuda'), g, m, v, *args)


# ------------------------------------------------------------------------------------------------- trainer

CFG3 = {'encoder.num_units': 16, 'decoder.num_units': 16, 'encoder.gemm_precision': 'f32', 'encoder.dropout': 1,
        'encoder.input_noise': 0, 'decoder.dropout': 1, 'decoder.sample_prob': 0, 'trainer.batch_size': 4}
# an equally small cfg1, its own regularisers left on: their draws come after the weight noise's
CFG1 = {'encoder.num_units': 16, 'encoder.gemm_precision': 'f32', 'trainer.batch_size': 4}
NOISE = {'trainer.weight_noise': 0.075}
CASES = {'cfg1': ('cfg1_dblstm_ctc', CFG1), 'cfg3': ('cfg3_las_vanilla', CFG3)}
SEED = 21


def _data(case, batches=100):
    if case == 'cfg1':
        return SyntheticData(4, 40, 40, min_frames=25, min_labels=2, max_labels=4, time_reduction=1, seed=2234,
                             batches_per_epoch=batches)
    return SyntheticData(4, 32, 40, num_labels=39, min_frames=20, min_labels=2, max_labels=5, eos=True, time_reduction=8,
                         seed=3234, batches_per_epoch=batches)


def _trainer(case, data, expdir=None, **over):
    recipe, base = CASES[case]
    mc, tc, ec = recipes.load_recipe(recipe, **dict(base, **over))
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=expdir,
                                               server=None, task_index=0)


def _params(tr):
    torch.cuda.synchronize()
    return {k: v.copy() for k, v in tr.model.store.state_dict().items()}


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_noisy_step_is_the_hand_made_noisy_step(case):
    data = _data(case)
    raw = data.batch(0)
    # A: the key
    nops.set_seed(SEED)
    A = _trainer(case, data, **NOISE)
    seen = {}
    A._create_graph()
    inner = A.loss_fn

    def watching(*a, **k):
        seen['flat'] = A.flat.clone()                # the parameters the forward pass ran at
        return inner(*a, **k)
    A.loss_fn = watching
    loss_a = A.step(A.to_device(raw))
    assert A.last_weight_noise == (SEED, 1) and not A._noisy
    seed, offset = A.last_weight_noise
    # B: no key; the test adds the same noise by hand, takes the offset A took, and restores before the plain Adam
    nops.set_seed(SEED)
    B = _trainer(case, data)
    B._create_graph()
    B._ensure_variables()
    B._init_optimizer()
    assert B.flat_clean is None
    initial = _params(B)
    clean = torch.empty_like(B.flat)
    assert nops.global_rng().next() == (seed, offset)
    table = hip.WeightNoiseTable(weight_noise_ranges(B.model.store.trainable_variables()), 'cuda')
    assert 0 < table.n < len(B.model.store.trainable_variables())
    hip.weight_noise(B.flat, clean, table, 0.075, seed, offset)
    plain_update = B._update

    def restore_then_update():
        B.flat.copy_(clean)
        plain_update()
    B._update = restore_then_update
    loss_b = B.step(B.to_device(raw))
    np.testing.assert_array_equal(bits(loss_a), bits(loss_b))
    pa, pb = _params(A), _params(B)
    _same(pa, pb)
    assert nops.global_rng().offset >= 1
    # C: no noise at all, the model's own draws at the offsets they had in A
    nops.set_seed(SEED)
    C = _trainer(case, data)
    nops.global_rng().next()
    loss_c = C.step(C.to_device(raw))
    assert float(loss_a.item()) != float(loss_c.item())
    assert np.isfinite(float(loss_a.item()))
    # the forward pass saw noisy matrices and clean vectors; afterwards every parameter is one Adam step from its
    # initial value (the first step moves an element by at most the learning rate), far less than the noise
    noisy = seen['flat'].cpu().numpy()
    lr = A.last_lr
    moved = 0
    for v in A.model.store.trainable_variables():
        during = noisy[v.offset:v.offset + v.numel()].reshape(v.shape)
        if len(v.shape) < 2:
            np.testing.assert_array_equal(bits(during), bits(initial[v.name]), err_msg=v.name)
        else:
            whole = v.numel() // 4 * 4
            d = (during.reshape(-1) - initial[v.name].reshape(-1))[:whole]
            assert np.mean(d != 0) > 0.9, v.name
            if whole >= 1024:                        # (the deviation of 1024 draws is within 2.2 % of sigma in 1 of 10^6)
                assert 0.06 < d.std() < 0.09, (v.name, d.std())
            moved += 1
        step = np.abs(pa[v.name].astype(np.float64) - initial[v.name])
        assert step.max() <= lr * (1 + 1e-5) + 2.0 ** -24 * np.abs(initial[v.name]).max(), (v.name, step.max(), lr)
    assert moved > 0 and lr < 0.01


def _run_steps(tr, data, steps):
    """the training loop's bookkeeping around step(): returns the losses' bits and the RNG offsets after each step"""
    out = []
    for s in range(steps):
        loss = tr.step(tr.to_device(data.batch(s)))
        tr.global_step += 1
        out.append((bits(loss).copy(), nops.global_rng().offset))
    return out


def test_start_step():
    data = _data('cfg3')
    nops.set_seed(SEED)
    plain = _trainer('cfg3', data)
    plain._create_graph()
    ref = _run_steps(plain, data, 2)
    after_two = _params(plain)
    ref += _run_steps(plain, data, 1)
    nops.set_seed(SEED)
    late = _trainer('cfg3', data, **dict(NOISE, **{'trainer.weight_noise_start_step': 2}))
    late._create_graph()
    got = _run_steps(late, data, 2)
    assert late.last_weight_noise is None
    for (la, oa), (lb, ob) in zip(ref, got):
        np.testing.assert_array_equal(la, lb)
        assert oa == ob                              # the stream did not move (CFG3 has no draws of its own: 0)
    _same(after_two, _params(late))
    got += _run_steps(late, data, 1)
    assert late.last_weight_noise == (SEED, ref[1][1] + 1)
    assert got[2][1] == ref[2][1] + 1                # one offset for the noisy step
    assert not np.array_equal(got[2][0], ref[2][0])
    a, b = _params(plain), _params(late)
    assert any(not np.array_equal(a[k], b[k]) for k in a)


def test_without_the_keys_the_step_makes_the_calls_it_always_made(monkeypatch):
    counts = {}
    for fname in ('weight_noise', 'adam_clip_step', 'adam_clip_step_from'):
        def counted(*a, _fn=getattr(hip, fname), _name=fname, **k):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(hip, fname, counted)
    data = _data('cfg3')
    nops.set_seed(SEED)
    tr = _trainer('cfg3', data)
    tr._create_graph()
    _run_steps(tr, data, 2)
    assert counts == {'adam_clip_step': 2}
    assert tr.flat_clean is None and tr.noise_table is None and nops.global_rng().offset == 0
    counts.clear()
    tr = _trainer('cfg3', data, **NOISE)
    tr._create_graph()
    _run_steps(tr, data, 2)
    assert counts == {'weight_noise': 2, 'adam_clip_step_from': 2}
    assert tr.flat_clean is not None and nops.global_rng().offset == 2


def test_a_step_that_raises_leaves_the_clean_parameters():
    data = _data('cfg3')
    nops.set_seed(SEED)
    tr = _trainer('cfg3', data, **NOISE)
    tr._create_graph()
    _run_steps(tr, data, 1)
    before, m_before = _params(tr), bits(tr.adam_m).copy()
    inner = tr.loss_fn
    state = {'raised': False, 'noisy': None}

    class Boom(Exception):
        pass

    def once(*a, **k):
        if not state['raised']:
            state['raised'] = True
            state['noisy'] = tr.flat.clone()
            raise Boom()
        return inner(*a, **k)
    tr.loss_fn = once
    with pytest.raises(Boom):
        tr.step(tr.to_device(data.batch(1)))
    assert not tr._noisy
    assert not np.array_equal(bits(state['noisy']), bits(tr.flat))          # the noise had been applied
    _same(before, _params(tr))
    np.testing.assert_array_equal(bits(tr.adam_m), m_before)
    loss = tr.step(tr.to_device(data.batch(1)))                             # the next step runs
    assert np.isfinite(float(loss.item()))
    after = _params(tr)
    assert any(not np.array_equal(before[k], after[k]) for k in before)


def test_noisy_run_resumes_bit_for_bit(tmp_path):
    """6 noisy steps of cfg2 with input noise and dropout on, interrupted after 3 and resumed from the checkpoint
    (tests/test_hip_regularisation.py, test_regularised_run_resumes_bit_for_bit, plus the key)"""
    over = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.num_epochs': 1, 'trainer.valid_frequency': 3,
            'evaluator.batch_size': 2, 'evaluator.numbatches': 2, 'encoder.input_noise': 0.6, 'encoder.dropout': 0.5,
            'trainer.weight_noise': 0.075}

    def trainer(expdir):
        data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11,
                             batches_per_epoch=6)
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
        return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                                   expdir=expdir, server=None, task_index=0)
    nops.set_seed(SEED)
    full = trainer(str(tmp_path / 'full'))
    hist = full.train()
    assert [h[0] for h in hist] == list(range(6)) and full.last_weight_noise is not None
    nops.set_seed(SEED)
    part = trainer(str(tmp_path / 'part'))
    part._create_graph()
    part._graph['num_steps'] = 6
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
    nops.global_rng().offset = 12345                  # whatever the process's RNG holds, the checkpoint decides
    cont = trainer(str(tmp_path / 'part'))
    hist2 = cont.train()
    assert [h[0] for h in hist2] == [3, 4, 5]
    np.testing.assert_array_equal(np.array([h[1] for h in hist2]), np.array([h[1] for h in hist[3:]]))
    _same(_params(full), _params(cont))
    assert cont.last_weight_noise == full.last_weight_noise


def test_the_overlapped_loop_gives_the_synchronous_history():
    def run(prefetch):
        over = dict(NOISE, **{'trainer.num_epochs': 1, 'evaluator.evaluator': 'None'})
        if prefetch:
            over['trainer.prefetch_batches'] = prefetch
        nops.set_seed(SEED)
        tr = _trainer('cfg3', _data('cfg3', batches=6), **over)
        return tr, tr.train()
    sync, hist = run(0)
    ahead, hist2 = run(2)
    assert len(hist) == 6 and hist2 == hist
    assert sync.last_weight_noise == ahead.last_weight_noise == (SEED, 6)
    _same(_params(sync), _params(ahead))


def test_two_ranks_on_one_gpu_end_with_identical_parameters(tmp_path):
    """two real ranks sharing the device (gloo group), each on its own batches, two noisy steps with the plain and two
    with the bucketed exchange: the update from the clean parameters keeps the replicas bit-identical"""
    import socket
    import subprocess
    import sys
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'weight_noise_two_ranks.py')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, script, str(tmp_path)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
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
        np.testing.assert_array_equal(bits(a[n]), bits(b[n]), err_msg=n)
    for mode in ('plain', 'buckets'):
        assert not np.array_equal(a['__losses_' + mode], b['__losses_' + mode])     # the ranks saw different batches
        assert np.isfinite(a['__losses_' + mode]).all()
        assert list(a['__noisy_' + mode]) == list(b['__noisy_' + mode]) == [1, 1]
    matrices = [n for n in names if n.startswith('buckets/') and a[n].ndim >= 2]
    assert matrices and all(not np.array_equal(a[n], a['__initial/' + n[8:]]) for n in matrices)
