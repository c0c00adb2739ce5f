"""Dropout and input noise against the host Philox reference (oracle/philox.py) and the float64 oracle given the
host's random numbers.

- nabu_dropout_f32 bit for bit against x * dropout_scale(...), nabu_gaussian_noise_f32 against x + s * gaussian(...)
  within a derived bound, seq_dropout's backward against dy * mask;
- one regularised training step of the DBLSTM and the Listener (input noise 0.6, keep 0.5, ragged lengths) and of
  the Speller (output dropout, alone and with scheduled sampling) on every dispatch path, against the oracle fed the
  masks and the noise the documented stream rules give:
    encoder: one RngState.next() per noise or dropout call, in the order the encoders make them, over the whole
             tensor (element e: lane e % 4 of group e // 4);
    decoder: layer n of step t uses stream (seed, offset * 1000003 + t * nl + n) over [B, U], element b * U + u;
- the RNG bookkeeping of two consecutive steps, counters whose high word is (or becomes) non-zero, and a resume of
  a regularised run from its checkpoint."""
import os

import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from oracle import philox as P
from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests.test_hip_speller import PRE, speller_params, grad_names

pytestmark = pytest.mark.gpu

rel = lambda a, b_: np.abs(a - b_).max() / (np.abs(b_).max() + 1e-12)


# ------------------------------------------------------------------------------------------ element-wise kernels

# past grid_for's cap of 2048 blocks x 256 threads x 4 elements, so the grid-stride loop takes a second lap
SIZES = [1, 3, 4, 5, 1023, 4099, 3000001]
# (seed, offset): small; both high words non-zero; offset 2^32 - 1 (the low word at its end)
STREAMS = [(7, 3), ((5 << 32) | 9, (3 << 32) | 1000003), ((1 << 40) + 3, (1 << 32) - 1)]
# storage offsets (floats) of x and y: (0, 0) takes the float4 path, every other pair the scalar one
PLACES = [(0, 0), (1, 1), (2, 3), (3, 0), (0, 2)]
SENTINEL = np.float32(-1234.5)


def _placed(n, host, off):
    """a device buffer of n + 8 floats holding `host` (or the sentinel) at float offset `off`, and that view"""
    buf = torch.full((n + 8,), float(SENTINEL), dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    if host is not None:
        v.copy_(torch.from_numpy(host))
    return buf, v


def _call(fn, n, x, y, a, seed, offset):
    from nabu_amd import _hip
    _hip.check(getattr(_hip.lib(), fn)(n, _hip.ptr(x), _hip.ptr(y), a, seed, offset, _hip.stream()), fn)


def _untouched_outside(buf, off, n):
    b = buf.cpu().numpy()
    assert np.all(b[:off] == SENTINEL) and np.all(b[off + n:] == SENTINEL)


@pytest.mark.parametrize('n', SIZES)
def test_dropout_kernel_is_bit_identical_to_the_host_mask(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n).astype(np.float32)
    for i, keep in enumerate([1.0, 0.9, 0.5, 0.1]):
        seed, offset = STREAMS[i % len(STREAMS)]
        s = P.dropout_scale(n, keep, seed, offset)
        want = np.where(s > 0, x * s, np.float32(0)).astype(np.float32)
        for xo, yo in (PLACES if n < 10 ** 6 else PLACES[:2]):
            _, xd = _placed(n, x, xo)
            ybuf, yd = _placed(n, None, yo)
            _call('nabu_dropout_f32', n, xd, yd, keep, seed, offset)
            got = yd.cpu().numpy()
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (keep, xo, yo, bad[:8], got[bad[:4]], want[bad[:4]])
            _untouched_outside(ybuf, yo, n)
        if keep < 1 and n >= 4099:
            assert abs((s > 0).mean() - keep) < 0.05


def test_dropout_kernel_every_stream_of_the_table():
    """each (seed, offset) of STREAMS at keep 0.5 on one ragged size: the key and counter words all count"""
    n = 4099
    x = np.random.default_rng(1).normal(size=n).astype(np.float32)
    outs = []
    for seed, offset in STREAMS + [(7, 3 + (1 << 32)), (7 + (1 << 32), 3)]:
        s = P.dropout_scale(n, 0.5, seed, offset)
        _, xd = _placed(n, x, 0)
        _, yd = _placed(n, None, 0)
        _call('nabu_dropout_f32', n, xd, yd, 0.5, seed, offset)
        got = yd.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), np.where(s > 0, x * s, np.float32(0)).view(np.uint32))
        outs.append(got)
    for i in range(len(outs)):
        for j in range(i):
            assert not np.array_equal(outs[i], outs[j]), (i, j)


def _noise_bound(z, rad, y, s):
    """|device - (x + s z)| allowed per element, z and y in float64.
    Box-Muller on the device: ra = sqrtf(-2 logf(u1)) (u1 exact; logf <= 1 ulp, sqrtf <= 0.5 ulp: <= 1.5 ulp of ra),
    sincosf(fl(fl32(2 pi) u)) (<= 2 ulp of the result at the float32 angle), z = ra * cos (0.5 ulp): <= 4 ulp of |z|,
    doubled to 8 * 2^-24 |z|.  The angle itself: |fl32(2 pi) - 2 pi| u <= 1.75e-7 plus the product's rounding
    <= 2.4e-7 (half an ulp at 2 pi): 4.2e-7 rad, which moves z by up to ra * 4.2e-7 -- taken as ra * 5e-7.  Then
    y = fl(x + fl(s z)): 2^-24 s |z| + 2^-24 |y|."""
    e = 2.0 ** -24
    return s * (8 * e * np.abs(z) + 5e-7 * rad) + e * s * np.abs(z) + e * np.abs(y) + 1e-30


@pytest.mark.parametrize('n', SIZES)
def test_gaussian_noise_kernel_against_the_host_box_muller(n):
    rng = np.random.default_rng(100 + n)
    x = rng.normal(size=n).astype(np.float32)
    for i, s in enumerate([0.6, 1.0]):
        seed, offset = STREAMS[(i + n) % len(STREAMS)]
        z, rad = P.gaussian(n, seed, offset, with_radius=True)
        want = x.astype(np.float64) + np.float64(np.float32(s)) * z
        tol = _noise_bound(z, rad, want, float(np.float32(s)))
        for xo, yo in (PLACES if n < 10 ** 6 else PLACES[:2]):
            _, xd = _placed(n, x, xo)
            ybuf, yd = _placed(n, None, yo)
            _call('nabu_gaussian_noise_f32', n, xd, yd, s, seed, offset)
            got = yd.cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            worst = int(err.argmax() if n else 0)
            assert np.all(err <= tol), (s, xo, yo, worst, err[worst], tol[worst], got[worst], want[worst])
            _untouched_outside(ybuf, yo, n)
    # stddev 0: an exact copy
    _, xd = _placed(n, x, 1)
    _, yd = _placed(n, None, 2)
    _call('nabu_gaussian_noise_f32', n, xd, yd, 0.0, *STREAMS[1])
    np.testing.assert_array_equal(yd.cpu().numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize('keep', [0.9, 0.5])
def test_seq_dropout_backward_regenerates_the_forward_mask(keep):
    from nabu_amd.autodiff import Tape, record
    from nabu_amd.neuralnetworks.components import ops as nops
    rng = np.random.default_rng(7)
    shape = (5, 37, 12)
    n = int(np.prod(shape))
    x = rng.normal(size=shape).astype(np.float32)
    dy = rng.normal(size=shape).astype(np.float32)
    rs = nops.RngState(seed=(3 << 32) | 11)
    rs.offset = (1 << 32) - 2
    src, xd = torch.tensor(x, device='cuda'), torch.tensor(x, device='cuda')
    with Tape() as tape:
        record([src], [xd], lambda g: [g])
        y = nops.seq_dropout(xd, keep, rs)
    assert (rs.seed, rs.offset) == ((3 << 32) | 11, (1 << 32) - 1)
    s = P.dropout_scale(n, keep, rs.seed, rs.offset).reshape(shape)
    np.testing.assert_array_equal(y.cpu().numpy().view(np.uint32),
                                  np.where(s > 0, x * s, np.float32(0)).astype(np.float32).view(np.uint32))
    dx = tape.ops[-1].backward(torch.tensor(dy, device='cuda'))[0].cpu().numpy()
    np.testing.assert_array_equal(dx.view(np.uint32),
                                  np.where(s > 0, dy * s, np.float32(0)).astype(np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------- encoders

CELL = 'bidirectional_rnn/%s/layer_norm_basic_lstm_cell/%s'


class StreamLog(object):
    """every nabu_amd.ops.dropout / gaussian_noise call: (kind, seed, offset, numel, phase)"""

    def __init__(self, monkeypatch):
        from nabu_amd import ops
        self.calls, self.phase = [], 'fwd'
        drop, noise = ops.dropout, ops.gaussian_noise

        def d(x, keep, seed, offset):
            self.calls.append(('drop', seed, offset, x.numel(), self.phase))
            return drop(x, keep, seed, offset)

        def g(x, s, seed, offset):
            self.calls.append(('noise', seed, offset, x.numel(), self.phase))
            return noise(x, s, seed, offset)
        monkeypatch.setattr(ops, 'dropout', d)
        monkeypatch.setattr(ops, 'gaussian_noise', g)

    def check(self, steps):
        """no two forward calls share a stream; each backward call uses a forward dropout call's stream and size,
        once; per step the forward calls take the offsets after the previous step's, one each"""
        fwd = [c for c in self.calls if c[4] == 'fwd']
        bwd = [c for c in self.calls if c[4] == 'bwd']
        streams = [(c[1], c[2]) for c in fwd]
        assert len(set(streams)) == len(streams), fwd
        fdrop = sorted((c[1], c[2], c[3]) for c in fwd if c[0] == 'drop')
        assert sorted((c[1], c[2], c[3]) for c in bwd) == fdrop, (fwd, bwd)
        assert all(c[0] == 'drop' for c in bwd)
        per = len(fwd) // steps
        offs = [c[2] for c in fwd]
        assert offs == list(range(offs[0], offs[0] + steps * per)), offs


def _enc_layers(st, enc, n):
    layers = []
    for l in range(n):
        pyr = enc == 'Listener' and l < n - 1
        pre = '%s/features/layer%d/%s' % (enc, l, 'BLSTM/' if pyr else '')
        layers.append({'%s_%s' % (d, w): st[pre + CELL % (d, w)].astype(np.float64)
                       for d in ('fw', 'bw') for w in ('kernel', 'bias')})
    return layers


def _enc_grad_names(enc, n):
    names = []
    for l in range(n):
        pyr = enc == 'Listener' and l < n - 1
        pre = '%s/features/layer%d/%s' % (enc, l, 'BLSTM/' if pyr else '')
        names.append({'%s_%s' % (d, w): pre + CELL % (d, w) for d in ('fw', 'bw') for w in ('kernel', 'bias')})
    return names


def _encoder_host_randoms(enc, x_shape, lens, H, nlayers, seed, off0, noise, keep):
    """the noise and masks the stream rules give: noise at off0 + 1, then one mask per layer"""
    B, T, D = x_shape
    off = off0 + 1
    nz = noise * P.gaussian(int(np.prod(x_shape)), seed, off).reshape(x_shape)
    shapes = []
    if enc == 'Listener':
        t = T
        for _ in range(nlayers - 1):
            t = -(-t // 2)
            shapes.append((B, t, 4 * H))
        shapes.append((B, t, 2 * H))
    else:
        shapes = [(B, T, 2 * H)] * nlayers
    masks = []
    for s in shapes:
        off += 1
        masks.append(P.dropout_scale(int(np.prod(s)), keep, seed, off).astype(np.float64).reshape(s))
    return nz, masks, off


def _oracle_ctc(enc, x, lens, y, yl, layers, W, b, noise=None, masks=None):
    fwd, bwd = (O.listener_fwd, O.listener_bwd) if enc == 'Listener' else (O.dblstm_fwd, O.dblstm_bwd)
    e, el, caches = fwd(x, lens, layers, noise=noise, masks=masks)
    lg = O.linear_fwd(e, W, b)
    nll, dlg = O.ctc_loss(lg, el, y, yl)
    de, dW, db = O.linear_bwd(dlg / x.shape[0], e, W)
    _, grads = bwd(de, caches)
    return nll.mean(), grads, dW, db


ENC_CASES = {
    # stepwise recurrent kernels
    'cfg1': ('cfg1_dblstm_ctc', 'DBLSTM', {'encoder.num_units': 32, 'trainer.batch_size': 4}, 40, 25, 1, 0),
    'cfg2': ('cfg2_listener_ctc', 'Listener', {'encoder.num_units': 32, 'trainer.batch_size': 4}, 64, 40, 8, 0),
    # H = 512, B = 32: the persistent plane kernels and the recipe's f16x3 products
    'cfg2_h512': ('cfg2_listener_ctc', 'Listener', {'trainer.batch_size': 32}, 32, 17, 8, 1),
    'cfg2_h512_f32': ('cfg2_listener_ctc', 'Listener', {'trainer.batch_size': 32, 'encoder.gemm_precision': 'f32',
                                                        'encoder.recurrent_precision': 'f32'}, 32, 17, 8, 1),
    'cfg1_h512': ('cfg1_dblstm_ctc', 'DBLSTM', {'trainer.batch_size': 32, 'encoder.num_units': 512}, 24, 9, 1, 1),
}


def _encoder_step(case, monkeypatch, off0=0, keep=0.5, noise=0.6, steps=1):
    """`steps` forward + backward passes of one batch at regularisation (noise, keep) from global RNG offset off0:
    the model's loss and gradients of the last step, its (seed, offset) before that step, the recurrent paths the
    layers took, the stream log, the batch and the model's state"""
    from nabu_amd import ops, _hip
    import ctypes
    from nabu_amd.autodiff import Tape
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.trainers import trainer_factory, loss_functions
    recipe, enc, over, T, minT, red, _ = ENC_CASES[case]
    over = dict(over, **{'encoder.input_noise': noise, 'encoder.dropout': keep})
    B = over['trainer.batch_size']
    data = SyntheticData(B, T, 40, min_frames=minT, min_labels=2, max_labels=4, time_reduction=red, seed=2234)
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                             expdir=None, server=None, task_index=0)
    raw = data.batch(0)
    batch = tr.to_device(raw)
    with torch.no_grad():           # create the variables (no regularisation outside training)
        tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'], batch['target_seq_length'], False)
    log = StreamLog(monkeypatch)
    paths = []
    fwd = ops.blstm_fwd

    def blstm_fwd(plan, *a):
        paths.append(_hip.lib().nabu_blstm_uses_persistent(ctypes.byref(plan.desc)))
        return fwd(plan, *a)
    monkeypatch.setattr(ops, 'blstm_fwd', blstm_fwd)
    rs = nops.global_rng()
    rs.offset = off0
    for _ in range(steps):
        for v in tr.model.store.vars.values():
            v.grad = None
        start = (rs.seed, rs.offset)
        log.phase = 'fwd'
        with Tape() as tape:
            logits, lsl = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'],
                                   batch['target_seq_length'], True)
            loss = loss_functions.CTC(batch['targets'], logits, lsl, batch['target_seq_length'])
        log.phase = 'bwd'
        tape.backward(loss)
    torch.cuda.synchronize()
    grads = {k: v.grad.cpu().numpy().astype(np.float64) for k, v in tr.model.store.vars.items() if v.grad is not None}
    return float(loss.item()), grads, start, paths, log, raw, tr.model.store.state_dict(), tr.model


def _check_encoder_against_oracle(case, monkeypatch, off0=0):
    recipe, enc, over, T, _, _, persistent = ENC_CASES[case]
    loss, grads, (seed, o), paths, log, raw, st, model = _encoder_step(case, monkeypatch, off0)
    assert o == off0
    nlayers = int(model.encoder.conf['num_layers']) + (1 if enc == 'Listener' else 0)
    H = int(model.encoder.conf['num_units'])
    assert paths == [persistent] * nlayers, paths
    x = raw['inputs']['features'].astype(np.float64)
    lens = raw['input_seq_length']['features']
    assert lens.min() < T                                    # ragged: padded frames get noise too
    y, yl = raw['targets']['text'], raw['target_seq_length']['text']
    nz, masks, last = _encoder_host_randoms(enc, x.shape, lens, H, nlayers, seed, off0, 0.6, 0.5)
    log.check(1)
    fwd = [c for c in log.calls if c[4] == 'fwd']
    assert [c[2] for c in fwd] == list(range(off0 + 1, last + 1))
    assert [c[3] for c in fwd] == [x.size] + [m.size for m in masks]
    assert [c[0] for c in fwd] == ['noise'] + ['drop'] * nlayers
    layers = _enc_layers(st, enc, nlayers)
    W = st['DNNDecoder/text/outlayer/weights'].astype(np.float64)
    b = st['DNNDecoder/text/outlayer/biases'].astype(np.float64)
    rloss, rg, rdW, rdb = _oracle_ctc(enc, x, lens, y, yl, layers, W, b, nz, masks)
    assert abs(loss - rloss) / abs(rloss) < 5e-5, (loss, rloss)
    for g, names in zip(rg, _enc_grad_names(enc, nlayers)):
        for k, name in names.items():
            assert rel(grads[name].reshape(g[k].shape), g[k]) < 3e-4, name
    assert rel(grads['DNNDecoder/text/outlayer/weights'].reshape(rdW.shape), rdW) < 3e-4
    assert rel(grads['DNNDecoder/text/outlayer/biases'].reshape(rdb.shape), rdb) < 3e-4
    # the regularisation really acted: the same step without it is O(1) away
    ploss, pg, _, _ = _oracle_ctc(enc, x, lens, y, yl, layers, W, b)
    assert abs(ploss - rloss) / abs(rloss) > 0.01 or rel(pg[0]['fw_kernel'], rg[0]['fw_kernel']) > 0.1
    assert rel(pg[0]['fw_kernel'], rg[0]['fw_kernel']) > 0.05


@pytest.mark.parametrize('case', sorted(ENC_CASES))
def test_regularised_encoder_step_matches_oracle(case, monkeypatch):
    _check_encoder_against_oracle(case, monkeypatch)


@pytest.mark.parametrize('case', ['cfg1', 'cfg2'])
def test_encoder_offset_crosses_the_low_word_between_layers(case, monkeypatch):
    """global offset 2^32 - 3: noise at 2^32 - 2, the first mask at 2^32 - 1, the next at 2^32"""
    _check_encoder_against_oracle(case, monkeypatch, off0=(1 << 32) - 3)


@pytest.mark.parametrize('case', ['cfg1', 'cfg2'])
def test_encoder_streams_over_two_steps(case, monkeypatch):
    """two consecutive training passes: every forward noise / dropout call has a stream of its own, across the
    steps too; every backward dropout call regenerates one forward call's stream"""
    *_, log, _, _, _ = _encoder_step(case, monkeypatch, off0=5, steps=2)
    log.check(2)
    assert sum(c[4] == 'bwd' for c in log.calls) > 0


def test_regularised_run_resumes_bit_for_bit(tmp_path):
    """cfg2 with input noise and dropout on, interrupted after 3 steps and resumed from its checkpoint: the same
    (step, loss) history and weights as the uninterrupted run -- what restoring rng_offset is for"""
    over = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.num_epochs': 1,
            'trainer.valid_frequency': 3, 'evaluator.batch_size': 2, 'evaluator.numbatches': 2,
            'encoder.input_noise': 0.6, 'encoder.dropout': 0.5}

    def trainer(expdir):
        data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11,
                             batches_per_epoch=6)
        from nabu_amd.neuralnetworks.trainers import trainer_factory
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
        return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                                   expdir=expdir, server=None, task_index=0)
    from nabu_amd.neuralnetworks.components import ops as nops
    # the RNG is the process's: both runs start from the same (seed, offset)
    nops.set_seed(21)
    full = trainer(str(tmp_path / 'full'))
    hist = full.train()
    assert [h[0] for h in hist] == list(range(6))
    assert nops.global_rng().offset > 0
    nops.set_seed(21)
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
    a, b = full.model.store.state_dict(), cont.model.store.state_dict()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------- decoder

class env(object):
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            os.environ[k] = v

    def __exit__(self, *a):
        for k in self.kv:
            os.environ.pop(k, None)


CHAIN = dict(NABU_SPELLER_PERSIST='0', NABU_SPELLER_PERSIST_BWD='0')


def _dec_data(rng, B, Te, E, C, tmin, tmax, scale=1.0):
    enc_len = rng.integers(Te // 2, Te + 1, B).astype(np.int32)
    enc_len[0] = Te
    tlen = rng.integers(tmin, tmax + 1, B).astype(np.int32)
    tlen[1] = tmax
    enc = (scale * rng.normal(size=(B, Te, E))).astype(np.float32)
    enc *= (np.arange(Te)[None, :, None] < enc_len[:, None, None])
    tg = rng.integers(0, C - 1, (B, tmax)).astype(np.int32)
    for b in range(B):
        tg[b, tlen[b] - 1] = C - 1
        tg[b, tlen[b]:] = 0
    return enc, enc_len, tg, tlen


def _dec_run(over, enc, enc_len, tg, tlen, C, seed, off0=0):
    """one forward + backward of a decoder built from the cfg3 recipe + over, the global RNG at (seed, off0):
    logits, d encoded, gradients, decoder inputs used [L, B], paths, the dropout stream's base offset, loss"""
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import Tape, SeqLen, record
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory, rnn_decoder
    from nabu_amd.neuralnetworks.trainers import loss_functions
    mc, _, _ = recipes.load_recipe('cfg3_las_vanilla', **over)
    dec = ed_decoder_factory.factory('speller')(mc, {'text': C}, None)
    store = vs.VariableStore(seed=3)
    dev = torch.device('cuda')
    nops.set_seed(seed)
    nops.global_rng().offset = off0
    enc_d, src, tgd = torch.tensor(enc, device=dev), torch.tensor(enc, device=dev), torch.tensor(tg, device=dev)
    with vs.as_default(store), Tape() as tape:
        record([src], [enc_d], lambda g: [g])
        logits, lsl, _ = dec({'features': enc_d}, {'features': SeqLen(enc_len, dev)}, {'text': tgd},
                             {'text': SeqLen(tlen, dev)}, True)
        loss = loss_functions.average_cross_entropy({'text': tgd}, logits, lsl, {'text': SeqLen(tlen, dev)})
    used = rnn_decoder.decoder_inputs().cpu().numpy().copy()
    paths = rnn_decoder.dynamic_decode.last_paths
    got = {}

    def capture(g):
        got['denc'] = g.cpu().numpy()
        return [None]
    tape.ops[0].backward = capture
    tape.backward(loss)
    st = store.state_dict()
    grads = {k: v.grad.cpu().numpy().copy() for k, v in store.vars.items() if v.grad is not None}
    return (logits['text'].cpu().numpy(), got['denc'], grads, used, paths, (off0 + 1) * 1000003,
            float(loss.item()), st)


def _decoder_masks(B, U, L, nl, keep, seed, base):
    return [[P.dropout_scale(B * U, keep, seed, base + t * nl + n).astype(np.float64).reshape(B, U)
             for n in range(nl)] for t in range(L)]


def check_decoder(over, enc, enc_len, tg, tlen, C, seed, off0=0, paths=None, tol=(2e-5, 1e-5, 2e-4)):
    nl = int(over['decoder.num_layers'])
    U = int(over['decoder.num_units'])
    keep = float(over['decoder.dropout'])
    attention = over['decoder.attention']
    window = None
    lg, denc, grads, used, got_paths, base, loss, st = _dec_run(over, enc, enc_len, tg, tlen, C, seed, off0)
    if paths is not None:
        assert got_paths == paths, got_paths
    B, L = len(tlen), int(tlen.max())
    masks = _decoder_masks(B, U, L, nl, keep, seed, base)
    p = speller_params(st, nl, attention)
    e64 = enc.astype(np.float64)
    rl, rll, cache = O.speller_fwd(e64, enc_len, tg, tlen, p, attention, dec_inputs=used.T, window=window,
                                   out_masks=masks)
    assert np.abs(lg - rl).max() < tol[0], np.abs(lg - rl).max()
    rloss, dlg = O.average_cross_entropy(rl, tg, rll, tlen)
    assert abs(loss - rloss) / rloss < tol[1], (loss, rloss)
    rdenc, rg = O.speller_bwd(dlg, cache)
    assert rel(denc, rdenc) < tol[2]
    for k, name in grad_names(nl, attention).items():
        assert rel(grads[name].astype(np.float64).reshape(rg[k].shape), rg[k]) < tol[2], k
    for n in range(nl):
        q = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        assert rel(grads[q + 'kernel'], rg['lstm'][n]['kernel']) < tol[2], n
        assert rel(grads[q + 'bias'], rg['lstm'][n]['bias']) < tol[2], n
    # the dropout really acted: the oracle without the masks is O(1) away
    plain = O.speller_fwd(e64, enc_len, tg, tlen, p, attention, dec_inputs=used.T, window=window)[0]
    assert np.abs(plain - rl).max() > 1e-2
    if float(over.get('decoder.sample_prob', 0)) > 0:
        teacher = np.concatenate([np.full((1, B), C - 1), tg[:, :L - 1].T], 0)
        live = np.arange(1, L)[:, None] < tlen[None, :]
        assert (used[1:] != teacher[1:])[live].any()          # some inputs really were drawn
    return got_paths


# (name, B, U, nl, attention, environment, expected (forward, backward) paths); encoder dim 64 except where noted
DEC_PATHS = [
    ('persistent_vanilla', 32, 64, 1, 'vanilla', {}, (1, 1)),
    ('persistent_location', 32, 64, 1, 'location_aware', {}, (1, 1)),
    # E = U = 128: rows16_ok(16, 4U, E + U, E) holds (E + U a multiple of 128), so the cell's product runs as
    # rows16_kernel with the output dropout in its epilogue
    ('chain_rows16', 32, 128, 1, 'vanilla', CHAIN, (0, 0)),
    ('chain_no_rows16', 32, 64, 1, 'vanilla', dict(CHAIN, NABU_SPELLER_ROWS16='0'), (0, 0)),
    ('chain_two_layers', 32, 64, 2, 'vanilla', CHAIN, (0, 0)),
    ('chain_four_subbatches', 64, 64, 1, 'location_aware', CHAIN, (0, 0)),
    # two sub-batches of 17: the second starts at row 17, element 17 U (a multiple of 4 since U is)
    ('chain_odd_subbatch_start', 34, 12, 1, 'vanilla', CHAIN, (0, 0)),
]
DEC_E = {'chain_rows16': 128}


def _dec_over(U, nl, attention, keep, sprob):
    over = {'decoder.num_layers': nl, 'decoder.num_units': U, 'decoder.attention': attention,
            'decoder.dropout': keep, 'decoder.sample_prob': sprob}
    if attention == 'location_aware':
        over.update({'decoder.numfilt': 3, 'decoder.filtersize': 7})
    return over


@pytest.mark.parametrize('keep,sprob', [(0.5, 0.0), (0.9, 0.0), (0.5, 0.5), (0.9, 0.1)])
@pytest.mark.parametrize('name,B,U,nl,attention,environ,paths', DEC_PATHS, ids=[d[0] for d in DEC_PATHS])
def test_regularised_decoder_matches_oracle(name, B, U, nl, attention, environ, paths, keep, sprob):
    rng = np.random.default_rng(B + U + nl + int(100 * keep))
    Te, E, C = 21, DEC_E.get(name, 64), 8
    enc, enc_len, tg, tlen = _dec_data(rng, B, Te, E, C, 3, 12, scale=0.5)
    from nabu_amd import ops as hip
    with env(**environ):
        check_decoder(_dec_over(U, nl, attention, keep, sprob), enc, enc_len, tg, tlen, C, seed=17 + B,
                      paths=paths)
    hip.check_persist_status()


def _crossing_off0(low):
    """a global offset o0 such that the dropout base (o0 + 1) * 1000003 has the low word `low` (mod 2^32)"""
    k = (low * pow(1000003, -1, 1 << 32)) % (1 << 32)
    assert (k * 1000003) % (1 << 32) == low
    return k - 1


@pytest.mark.parametrize('name', ['persistent_vanilla', 'chain_rows16', 'chain_no_rows16', 'chain_two_layers'])
def test_decoder_masks_cross_the_high_counter_word(name):
    """the dropout base offset 5 below a multiple of 2^32: the masks of the later steps (and, with two layers,
    the later layers) take the next high word"""
    _, B, U, nl, attention, environ, paths = [d for d in DEC_PATHS if d[0] == name][0]
    rng = np.random.default_rng(77)
    Te, E, C = 21, DEC_E.get(name, 64), 8
    enc, enc_len, tg, tlen = _dec_data(rng, B, Te, E, C, 3, 12, scale=0.5)
    off0 = _crossing_off0((1 << 32) - 5)
    base = (off0 + 1) * 1000003
    assert base >> 32 != (base + int(tlen.max()) * nl) >> 32
    from nabu_amd import ops as hip
    with env(**environ):
        check_decoder(_dec_over(U, nl, attention, 0.5, 0.5), enc, enc_len, tg, tlen, C, seed=(9 << 32) | 1,
                      off0=off0, paths=paths)
    hip.check_persist_status()


def test_decoder_refuses_units_that_would_split_a_dropout_group():
    """U % 4 != 0 would start a sub-batch inside a 4-element group of the mask (B = 34, U = 10: row 17 at element
    170): the decoder refuses the shape"""
    from nabu_amd import _hip
    rng = np.random.default_rng(3)
    enc, enc_len, tg, tlen = _dec_data(rng, 34, 9, 16, 8, 2, 5)
    with env(**CHAIN):
        with pytest.raises(_hip.NabuHipError, match='multiples of 4'):
            _dec_run(_dec_over(10, 1, 'vanilla', 0.5, 0.0), enc, enc_len, tg, tlen, 8, seed=1)


def test_regularised_decoder_at_the_cfg3_geometry_matches_oracle():
    """the full decoder geometry of BASELINE configs[2] (32 utterances, 125 frames of 1024 features, 512 units,
    40 classes, up to 60 steps) at the training defaults (output dropout 0.9, sample_prob 0.1) on the persistent
    launch: logits, loss and every gradient against the oracle given the host's masks and the inputs drawn"""
    rng = np.random.default_rng(43)
    B, Te, E, C, U = 32, 125, 1024, 40, 512
    enc, enc_len, tg, tlen = _dec_data(rng, B, Te, E, C, 20, 60, scale=0.3)
    from nabu_amd import ops as hip
    check_decoder(_dec_over(U, 1, 'vanilla', 0.9, 0.1), enc, enc_len, tg, tlen, C, seed=5, paths=(1, 1))
    hip.check_persist_status()
