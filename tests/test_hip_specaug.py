"""SpecAugment on the device (nabu_spec_augment_f32) against the host reference (tests/specaug_ref.py):

- the parameter buffer equals the host's draws exactly, over the stream table of test_hip_regularisation.py, at the
  lengths around the warp's threshold n = 2 W + 3 and with caps that bind (ratio, widths larger than n / the block);
- masks only: the result is bit-identical to the host's, x and y at every float offset inside sentinel-filled buffers;
- warp: within a bound derived from the two roundings of the interpolation; frames 0, c', n - 1 bit-exact;
- through the recipe API (a shrunken Listener at the cfg2 geometry, the DBLSTM): a step with the policy on equals the
  same model, policy off, fed the host-augmented features; the stream bookkeeping next to input_noise; validation
  untouched; reproducibility from ops.set_seed; a resumed run continues with the same draws."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import philox as P
from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests import specaug_ref as R
from tests.test_hip_regularisation import STREAMS, SENTINEL, _placed, _untouched_outside, _noise_bound, rel

pytestmark = pytest.mark.gpu

B_MAX, T_MAX = 6, 37
U = 2.0 ** -24          # unit roundoff of float32


def _policy(p):
    from nabu_amd import ops
    return ops.SpecAugmentPolicy(*p)


def _raw_call(x, len_dev, y, pol, seed, offset, params=None):
    """nabu_spec_augment_f32 on caller-placed buffers (ops.spec_augment allocates its own output)"""
    from nabu_amd import _hip
    B, T, D = x.shape
    d = _hip.SpecAugDesc(ctypes.sizeof(_hip.SpecAugDesc), B, T, D, pol.feature_blocks, pol.time_warp, pol.time_masks,
                         pol.time_mask_width, pol.freq_masks, pol.freq_mask_width, pol.time_mask_ratio)
    _hip.check(_hip.lib().nabu_spec_augment_f32(ctypes.byref(d), _hip.ptr(x), _hip.ptr(len_dev), _hip.ptr(y),
                                                _hip.ptr(params), seed, offset, _hip.stream()), 'nabu_spec_augment_f32')


def _features(rng, B, T, D, lens):
    """normal features shifted off zero (a zero in the result is a mask's), zero past the length as the pipelines pad"""
    x = (rng.normal(size=(B, T, D)) + np.where(rng.random((B, T, D)) < 0.5, 3, -3)).astype(np.float32)
    return x * (np.arange(T)[None, :, None] < np.asarray(lens)[:, None, None])


# ------------------------------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize('W', [1, 5])
def test_parameter_buffer_equals_the_host_draws(W):
    from nabu_amd import ops
    T, D = T_MAX, 12
    lens = np.array([1, 2, 2 * W + 2, 2 * W + 3, T], np.int32)
    x = torch.zeros((len(lens), T, D), device='cuda')
    ld = torch.tensor(lens, device='cuda')
    warped = 0
    # (time_mask_width, ratio, freq_mask_width, blocks): the ratio binds (0.2 n < 6); nothing binds; widths larger than
    # n and than the block of 4 columns bind
    for Tw, ratio, Fw, blocks in [(6, 0.2, 3, 1), (6, 1.0, 3, 1), (50, 1.0, 9, 3), (50, 0.2, 9, 3)]:
        for seed, offset in STREAMS:
            pol = _policy((W, 2, Tw, ratio, 2, Fw, blocks))
            prm = torch.full((len(lens), pol.param_width), -7, dtype=torch.int32, device='cuda')
            ops.spec_augment(x, ld, pol, seed, offset, params=prm)
            want = R.params(lens, D, pol, seed, offset)
            np.testing.assert_array_equal(prm.cpu().numpy(), want, err_msg=str((Tw, ratio, Fw, blocks, seed, offset)))
            assert (want[:3, :2] == 0).all() and (want[3:, 0] > 0).all()     # n = 2 W + 3 is the first length warped
            warped += int((want[:, 0] != want[:, 1]).sum())
    assert warped > 0


@pytest.mark.parametrize('D,blocks', [(1, 1), (3, 1), (5, 1), (40, 1), (123, 3)])
def test_masks_only_is_bit_identical_to_the_host(D, blocks):
    B, T = B_MAX, T_MAX
    rng = np.random.default_rng(D)
    lens = np.array([T, 1, 20, 36, 0, 9], np.int32)
    x = _features(rng, B, T, D, lens)
    x[2, 20:] = 5.0                  # something past a length: padding is copied, not cleaned
    n = B * T * D
    ld = torch.tensor(lens, device='cuda')
    pol = _policy((0, 2, 10, 1.0, 2, max(1, D // blocks // 3), blocks))
    for k, (xo, yo) in enumerate((a, b) for a in range(4) for b in range(4)):
        seed, offset = STREAMS[k % len(STREAMS)]
        want, prm, frac, _ = R.augment(x, lens, pol, seed, offset)
        assert not frac.any()
        want = want.astype(np.float32)
        _, xd = _placed(n, x.reshape(-1), xo)
        ybuf, yd = _placed(n, None, yo)
        pd = torch.zeros(prm.shape, dtype=torch.int32, device='cuda')
        _raw_call(xd.view(B, T, D), ld, yd.view(B, T, D), pol, seed, offset, pd)
        got = yd.cpu().numpy().reshape(B, T, D)
        np.testing.assert_array_equal(pd.cpu().numpy(), prm)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (xo, yo, bad[:6], got[tuple(bad[0])], want[tuple(bad[0])])
        _untouched_outside(ybuf, yo, n)
        for b in range(B):
            np.testing.assert_array_equal(got[b, lens[b]:], x[b, lens[b]:])
    # the masks did something at this size: some frames and some columns are zero
    if D >= 5:
        assert (want[0] == 0).all(1).any() or (want[3] == 0).all(1).any()
        assert any((want[b, :lens[b]] == 0).all(0).any() for b in (0, 2, 3))


def _warp_bound(y, span):
    """|device - host| allowed per element of a warped frame; y, span = frac |b - a| from the host in float64.
    The device evaluates fmaf(frac, fl(b - a), a) with the float32 frac the host uses (r, den < 2^24 convert exactly
    and the division is correctly rounded on both sides).  d = fl(b - a) carries one rounding, |d - (b - a)| <=
    u |b - a|, which reaches the result scaled by frac: u span.  The fma rounds once more: u |frac d + a| <=
    u (|y| + u span).  Sum: u (span + |y|) to first order, doubled as _noise_bound doubles its count of roundings:
    2 u (span + |y|), plus the smallest subnormal for results that underflow.  Where r = 0 (span = 0 and y = a) and
    inside the masks the host's value is exact and the bound is not used: those elements are compared bit for bit."""
    return 2 * U * (span + np.abs(y)) + 2.0 ** -149


@pytest.mark.parametrize('D,blocks', [(3, 1), (5, 1), (123, 3)])
@pytest.mark.parametrize('masks', [0, 2])
def test_warp_against_the_host_interpolation(D, blocks, masks):
    B, T = B_MAX, T_MAX
    rng = np.random.default_rng(10 * D + masks)
    n = B * T * D
    for k, W in enumerate([1, 5]):
        lens = np.array([T, 2 * W + 3, 2 * W + 2, 30, T - 1, 2 * W + 4], np.int32)
        x = _features(rng, B, T, D, lens)
        ld = torch.tensor(lens, device='cuda')
        pol = _policy((W, masks, 4, 1.0, masks, max(1, D // blocks // 4), blocks))
        seed, offset = STREAMS[(k + D) % len(STREAMS)]
        want, prm, frac, span = R.augment(x, lens, pol, seed, offset)
        assert (prm[[0, 1, 3, 4, 5], 0] > 0).all() and tuple(prm[2, :2]) == (0, 0)
        assert (frac > 0).any() and (prm[:, 0] != prm[:, 1]).any()   # a real warp: fractional positions
        xo, yo = (k + D) % 4, (2 * k + 1) % 4
        _, xd = _placed(n, x.reshape(-1), xo)
        ybuf, yd = _placed(n, None, yo)
        pd = torch.zeros(prm.shape, dtype=torch.int32, device='cuda')
        _raw_call(xd.view(B, T, D), ld, yd.view(B, T, D), pol, seed, offset, pd)
        got = yd.cpu().numpy().reshape(B, T, D)
        np.testing.assert_array_equal(pd.cpu().numpy(), prm)
        _untouched_outside(ybuf, yo, n)
        err = np.abs(got.astype(np.float64) - want)
        tol = _warp_bound(want, span)
        worst = tuple(int(i) for i in np.unravel_index((err / tol).argmax(), err.shape))
        print('D %d W %d masks %d: largest err / bound %.3f at %s (err %.3e, bound %.3e)'
              % (D, W, masks, (err / tol)[worst], worst, err[worst], tol[worst]))
        assert (err <= tol).all(), (worst, got[worst], want[worst], err[worst], tol[worst])
        # where the host's value is exact the device's is the same float32
        exact = np.broadcast_to((frac == 0)[:, :, None], got.shape) | (want == 0)
        np.testing.assert_array_equal(got[exact], want.astype(np.float32)[exact])
        if masks == 0:
            for b in np.flatnonzero(prm[:, 0] > 0):
                c, cp, nb = int(prm[b, 0]), int(prm[b, 1]), int(lens[b])
                for t, src in ((0, 0), (cp, c), (nb - 1, nb - 1)):
                    np.testing.assert_array_equal(got[b, t].view(np.uint32), x[b, src].view(np.uint32))
            np.testing.assert_array_equal(got[2], x[2])             # n = 2 W + 2: too short, copied


def test_off_is_an_exact_copy():
    from nabu_amd import ops
    rng = np.random.default_rng(4)
    lens = np.array([T_MAX, 5, 0], np.int32)
    x = torch.tensor(rng.normal(size=(3, T_MAX, 7)).astype(np.float32), device='cuda')
    ld = torch.tensor(lens, device='cuda')
    for p in [(0, 0, 0, 1.0, 0, 0, 1), (0, 2, 0, 1.0, 2, 0, 1), (0, 0, 9, 0.5, 0, 9, 7)]:
        pol = _policy(p)
        prm = torch.full((3, pol.param_width), -1, dtype=torch.int32, device='cuda')
        y = ops.spec_augment(x, ld, pol, 5, 6, params=prm)
        assert y.data_ptr() != x.data_ptr()
        np.testing.assert_array_equal(y.cpu().numpy().view(np.uint32), x.cpu().numpy().view(np.uint32))
        got = prm.cpu().numpy()
        assert (got[:, :2] == 0).all() and (got[:, 3::2] == 0).all()         # not warped; every width 0


def test_features_that_need_a_gradient_are_refused():
    from nabu_amd import ops
    from nabu_amd.autodiff import Tape, record
    from nabu_amd.neuralnetworks.components import ops as nops
    src, x = torch.zeros((2, 5, 4), device='cuda'), torch.zeros((2, 5, 4), device='cuda')
    rs = nops.RngState(1)
    with Tape():
        record([src], [x], lambda g: [g])
        with pytest.raises(Exception, match='gradient'):
            nops.spec_augment(x, np.array([5, 3], np.int32), ops.SpecAugmentPolicy(time_masks=1, time_mask_width=2), rs)
    assert rs.offset == 0


# ------------------------------------------------------------------------------------------------- recipe API

# recipe, encoder overrides, T, shortest utterance, time reduction
MODELS = {
    'listener': ('cfg2_listener_ctc', 32, 17, 8),
    'dblstm': ('cfg1_dblstm_ctc', T_MAX, 20, 1),
}
MASKS = {'encoder.time_masks': 2, 'encoder.time_mask_width': 6, 'encoder.time_mask_ratio': 0.5,
         'encoder.freq_masks': 2, 'encoder.freq_mask_width': 7}
WARP = dict(MASKS, **{'encoder.time_warp': 4})
SEED = (3 << 32) | 11


class AugLog(object):
    """every nabu_amd.ops.spec_augment / gaussian_noise call of the encoders, with what was drawn"""

    def __init__(self, monkeypatch):
        from nabu_amd import ops
        self.calls = []
        aug, noise = ops.spec_augment, ops.gaussian_noise

        def a(x, len_dev, policy, seed, offset, params=None):
            prm = torch.zeros((x.shape[0], policy.param_width), dtype=torch.int32, device=x.device)
            y = aug(x, len_dev, policy, seed, offset, prm)
            self.calls.append(dict(kind='aug', seed=seed, offset=offset, x=x, y=y, params=prm.cpu().numpy(), policy=policy))
            return y

        def g(x, s, seed, offset):
            y = noise(x, s, seed, offset)
            self.calls.append(dict(kind='noise', seed=seed, offset=offset, x=x, y=y, stddev=s))
            return y
        monkeypatch.setattr(ops, 'spec_augment', a)
        monkeypatch.setattr(ops, 'gaussian_noise', g)

    def aug(self):
        return [c for c in self.calls if c['kind'] == 'aug']


def _trainer(model, over, B=4, expdir=None, batches=100):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    recipe, T, minT, red = MODELS[model]
    over = dict({'encoder.num_units': 16, 'trainer.batch_size': B, 'encoder.dropout': 1, 'encoder.input_noise': 0}, **over)
    data = SyntheticData(B, T, 40, min_frames=minT, min_labels=2, max_labels=3, time_reduction=red, seed=2234,
                         batches_per_epoch=batches)
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=expdir,
                                               server=None, task_index=0), data


def _step(model, over, feats=None, seed=SEED, off0=0, steps=1, training=True):
    """`steps` forward + backward passes of batch 0 (its features replaced by `feats`) with the process's RNG at
    (seed, off0): loss, gradients and logits of the last pass, the RNG offset afterwards, the raw batch"""
    from nabu_amd.autodiff import Tape
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.trainers import loss_functions
    tr, data = _trainer(model, over)
    raw = data.batch(0)
    if feats is not None:
        raw['inputs']['features'] = feats
    batch = tr.to_device(raw)
    with torch.no_grad():           # create the variables (validation: no regularisation)
        tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'], batch['target_seq_length'], False)
    nops.set_seed(seed)
    nops.global_rng().offset = off0
    if not training:
        with torch.no_grad():
            logits, _ = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'],
                                 batch['target_seq_length'], False)
        return None, None, logits['text'].cpu().numpy(), nops.global_rng().offset, raw
    for _ in range(steps):
        for v in tr.model.store.vars.values():
            v.grad = None
        with Tape() as tape:
            logits, lsl = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'],
                                   batch['target_seq_length'], True)
            loss = loss_functions.CTC(batch['targets'], logits, lsl, batch['target_seq_length'])
        tape.backward(loss)
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy() for k, v in tr.model.store.vars.items() if v.grad is not None}
    return float(loss.item()), grads, logits['text'].cpu().numpy(), nops.global_rng().offset, raw


def _host_augmented(raw, over, seed, offset):
    from nabu_amd.neuralnetworks.models.ed_encoders.listener import spec_augment_keys
    pol = spec_augment_keys({k.split('.')[1]: str(v) for k, v in over.items()})
    y, prm, frac, _ = R.augment(raw['inputs']['features'], raw['input_seq_length']['features'], pol, seed, offset)
    return y.astype(np.float32), prm, frac


@pytest.mark.parametrize('model', sorted(MODELS))
def test_masked_step_equals_the_plain_step_on_host_masked_features(model, monkeypatch):
    log = AugLog(monkeypatch)
    loss, grads, logits, off, raw = _step(model, MASKS)
    assert off == 1 and [(c['seed'], c['offset']) for c in log.aug()] == [(SEED, 1)]
    feats, prm, frac = _host_augmented(raw, MASKS, SEED, 1)
    np.testing.assert_array_equal(log.aug()[0]['params'], prm)
    np.testing.assert_array_equal(log.aug()[0]['y'].cpu().numpy().view(np.uint32), feats.view(np.uint32))
    x = raw['inputs']['features']
    assert not frac.any() and (feats != x).mean() > 0.02                   # the masks really acted
    del log.calls[:]
    ploss, pgrads, plogits, poff, _ = _step(model, {}, feats=feats)
    assert poff == 0 and not log.calls
    assert loss == ploss
    np.testing.assert_array_equal(logits, plogits)
    assert sorted(grads) == sorted(pgrads) and len(grads) >= 6
    for k in grads:
        np.testing.assert_array_equal(grads[k], pgrads[k], err_msg=k)
    # and the unmasked step is somewhere else
    uloss, _, _, _, _ = _step(model, {})
    assert abs(uloss - loss) / abs(loss) > 1e-4


@pytest.mark.parametrize('model', sorted(MODELS))
def test_warped_step_matches_the_plain_step_on_host_warped_features(model, monkeypatch):
    log = AugLog(monkeypatch)
    loss, grads, _, off, raw = _step(model, WARP, off0=(1 << 32) - 2)
    assert off == (1 << 32) - 1
    feats, prm, frac = _host_augmented(raw, WARP, SEED, (1 << 32) - 1)
    np.testing.assert_array_equal(log.aug()[0]['params'], prm)
    assert (prm[:, 0] > 0).all() and (frac > 0).any()
    ploss, pgrads, _, _, _ = _step(model, {}, feats=feats)
    # (the tolerances of test_hip_regularisation.py's regularised steps against their reference)
    assert abs(loss - ploss) / abs(ploss) < 5e-5, (loss, ploss)
    for k in grads:
        assert rel(grads[k].astype(np.float64), pgrads[k].astype(np.float64)) < 3e-4, k


@pytest.mark.parametrize('model', sorted(MODELS))
def test_noise_keeps_its_offset_and_the_augmentation_takes_the_next(model, monkeypatch):
    log = AugLog(monkeypatch)
    over = dict(MASKS, **{'encoder.input_noise': 0.6})
    _, _, _, off, raw = _step(model, over, off0=5)
    assert off == 7 and [(c['kind'], c['seed'], c['offset']) for c in log.calls] == [('noise', SEED, 6), ('aug', SEED, 7)]
    noise, aug = log.calls
    x = raw['inputs']['features']
    # the noise is the one a configuration without the new keys draws: the whole tensor at offset off0 + 1
    z, rad = P.gaussian(x.size, SEED, 6, with_radius=True)
    s = float(np.float32(0.6))
    want = x.reshape(-1).astype(np.float64) + s * z
    noisy = noise['y'].cpu().numpy()
    assert np.all(np.abs(noisy.reshape(-1).astype(np.float64) - want) <= _noise_bound(z, rad, want, s))
    del log.calls[:]
    _step(model, {'encoder.input_noise': 0.6}, off0=5)
    assert [(c['kind'], c['offset']) for c in log.calls] == [('noise', 6)]
    np.testing.assert_array_equal(log.calls[0]['y'].cpu().numpy(), noisy)
    # the augmentation reads the noisy features (padding included: it carries noise too) at the next offset
    assert aug['x'] is noise['y']
    pol = aug['policy']
    y, prm, _, _ = R.augment(noisy, raw['input_seq_length']['features'], pol, SEED, 7)
    np.testing.assert_array_equal(aug['params'], prm)
    np.testing.assert_array_equal(aug['y'].cpu().numpy().view(np.uint32), y.astype(np.float32).view(np.uint32))


def test_all_keys_zero_makes_no_call_and_takes_no_offset(monkeypatch):
    log = AugLog(monkeypatch)
    zero = {'encoder.time_warp': 0, 'encoder.time_masks': 0, 'encoder.freq_masks': 0, 'encoder.time_mask_width': 9,
            'encoder.freq_mask_width': 9, 'encoder.feature_blocks': 1}
    loss, grads, _, off, _ = _step('listener', zero, off0=3)
    assert off == 3 and not log.calls
    ploss, pgrads, _, _, _ = _step('listener', {}, off0=3)
    assert loss == ploss
    for k in grads:
        np.testing.assert_array_equal(grads[k], pgrads[k], err_msg=k)


def test_validation_leaves_the_features_untouched(monkeypatch):
    log = AugLog(monkeypatch)
    _, _, logits, off, _ = _step('listener', WARP, off0=3, training=False)
    assert off == 3 and not log.calls
    _, _, plogits, _, _ = _step('listener', {}, off0=3, training=False)
    np.testing.assert_array_equal(logits, plogits)


def test_seed_reproduces_a_step_and_consecutive_steps_differ(monkeypatch):
    log = AugLog(monkeypatch)
    loss, grads, _, off, _ = _step('listener', WARP, seed=21, steps=2)
    first, second = log.aug()
    assert off == 2 and (first['offset'], second['offset']) == (1, 2)
    assert not np.array_equal(first['params'], second['params'])
    assert not np.array_equal(first['y'].cpu().numpy(), second['y'].cpu().numpy())
    del log.calls[:]
    loss2, grads2, _, _, _ = _step('listener', WARP, seed=21, steps=2)
    assert loss == loss2
    np.testing.assert_array_equal(log.aug()[1]['params'], second['params'])
    for k in grads:
        np.testing.assert_array_equal(grads[k], grads2[k], err_msg=k)
    del log.calls[:]
    _step('listener', WARP, seed=22, steps=1)
    assert not np.array_equal(log.aug()[0]['params'], first['params'])


def test_resumed_run_continues_with_the_same_draws(tmp_path, monkeypatch):
    """two steps of an augmented run, and the same run stopped after step 1 and resumed from its checkpoint: step 2
    draws the same warp and masks, and ends at the same loss and weights"""
    from nabu_amd.neuralnetworks.components import ops as nops
    log = AugLog(monkeypatch)
    over = dict(WARP, **{'trainer.num_epochs': 1, 'trainer.valid_frequency': 3, 'evaluator.batch_size': 2,
                         'evaluator.numbatches': 1, 'trainer.batch_size': 3})
    nops.set_seed(21)
    full, _ = _trainer('listener', over, B=3, expdir=str(tmp_path / 'full'), batches=2)
    hist = full.train()
    assert [h[0] for h in hist] == [0, 1] and nops.global_rng().offset == 2
    draws = [c['params'] for c in log.aug()]
    assert len(draws) == 2 and not np.array_equal(draws[0], draws[1])
    del log.calls[:]
    nops.set_seed(21)
    part, _ = _trainer('listener', over, B=3, expdir=str(tmp_path / 'part'), batches=2)
    part.checkpoint_steps = 1
    orig = type(part).step
    calls = {'n': 0}

    class Stop(Exception):
        pass

    def step_then_stop(self, batch):
        if calls['n'] == 1:
            raise Stop()
        calls['n'] += 1
        return orig(self, batch)
    monkeypatch.setattr(type(part), 'step', step_then_stop)
    with pytest.raises(Stop):
        part.train()
    monkeypatch.setattr(type(part), 'step', orig)
    np.testing.assert_array_equal(log.aug()[0]['params'], draws[0])
    del log.calls[:]
    nops.global_rng().offset = 12345                  # whatever the process's RNG holds, the checkpoint decides
    cont, _ = _trainer('listener', over, B=3, expdir=str(tmp_path / 'part'), batches=2)
    hist2 = cont.train()
    assert [h[0] for h in hist2] == [1] and hist2[0][1] == hist[1][1]
    assert [c['offset'] for c in log.aug()] == [2]
    np.testing.assert_array_equal(log.aug()[0]['params'], draws[1])
    a, b = full.model.store.state_dict(), cont.model.store.state_dict()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
