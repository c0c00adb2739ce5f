"""GPU: label smoothing for the cross-entropy losses against the float64 reference (tests/xent_smooth_ref.py): the two
kernels (xent_kernel<SMOOTH> up to 1023 classes, wide_rows_kernel<XENT, VEC, SMOOTH> from 1024) through their new
entry points, the loss functions on a model's logits, and the trainer key `label_smoothing`.

The bars are the ones these kernels have always been held to (test_hip_dnn.test_wide_cross_entropy): norm-wise
rel(loss) <= 1e-6 and rel(dlogits) <= 1e-5."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip
from nabu_amd import ops as hip
from nabu_amd import recipes
from nabu_amd.autodiff import SeqLen, Tape, record
from nabu_amd.neuralnetworks.trainers import loss_functions, trainer_factory
from nabu_amd.processing.synthetic import SyntheticData
from tests import xent_smooth_ref as R

pytestmark = pytest.mark.gpu

LOSS_BAR, GRAD_BAR = 1e-6, 1e-5
B, L = 5, 19
LOGIT_LEN = np.array([19, 4, 11, 1, 0], np.int32)
TARGET_LEN = np.array([19, 4, 11, 1, 3], np.int32)
SCALE = 0.2
SENTINEL = -12345.5
PAD = 64                                           # floats of sentinel on either side of an output

rel = lambda a, b_: float(np.abs(np.asarray(a, np.float64) - b_).max() / (np.abs(b_).max() + 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _case(C, L_=L, seed=None, lens=(LOGIT_LEN, TARGET_LEN)):
    rng = np.random.default_rng(C if seed is None else seed)
    logits = (3 * rng.standard_normal((B, L_, C))).astype(np.float32)
    targets = rng.integers(0, C, (B, L_ + 2)).astype(np.int32)
    return logits, targets, lens[0], lens[1]


def _framed(numel, phase=0):
    """a sentinel-filled buffer and the view of `numel` floats inside it, `phase` floats off a 16-byte boundary"""
    buf = torch.full((numel + 2 * PAD + 4,), SENTINEL, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + phase:PAD + phase + numel]


def _untouched(buf, numel, phase=0):
    b = host(buf)
    return np.all(b[:PAD + phase] == SENTINEL) and np.all(b[PAD + phase + numel:] == SENTINEL)


def _raw(wide, logits, targets, ll, tl, smoothing, phase=0, scale=SCALE):
    """the entry point itself, loss and dlogits placed inside sentinel-filled buffers: (loss, dlogits) and whether
    everything outside them was left alone"""
    lib = _hip.lib()
    Bn, Ln, C = logits.shape
    lbuf, loss = _framed(Bn)
    dbuf, dl = _framed(Bn * Ln * C, phase)
    args = [Bn, Ln, C, targets.shape[1], _hip.ptr(logits), _hip.ptr(targets), _hip.ptr(ll), _hip.ptr(tl), scale,
            smoothing, _hip.ptr(loss), _hip.ptr(dl)]
    if wide:
        ws_bytes = lib.nabu_xent_wide_ws_bytes(Bn, Ln)
        wbuf, ws = _framed(ws_bytes // 4)
        _hip.check(lib.nabu_xent_wide_smooth_loss_grad(*(args + [_hip.ptr(ws), ws_bytes, _hip.stream()])), 'wide smooth')
    else:
        _hip.check(lib.nabu_xent_smooth_loss_grad(*(args + [_hip.stream()])), 'smooth')
    torch.cuda.synchronize()
    clean = _untouched(lbuf, Bn) and _untouched(dbuf, Bn * Ln * C, phase)
    if wide:
        clean = clean and _untouched(wbuf, ws_bytes // 4)
    return loss.clone(), dl.clone().view(Bn, Ln, C), clean


def _check(loss, dl, logits, targets, ll, tl, e, scale=SCALE):
    per, g = R.average(logits, targets, ll, tl, e, grad_scale=scale)
    rl, rg = rel(host(loss), per), rel(host(dl), g)
    print('C=%d L=%d e=%g: rel(loss) %.3g, rel(dlogits) %.3g' % (logits.shape[2], logits.shape[1], e, rl, rg))
    assert rl <= LOSS_BAR, rl
    assert rg <= GRAD_BAR, rg
    d = host(dl)
    n = np.clip(ll, 0, logits.shape[1])
    for b in range(len(n)):
        assert not d[b, n[b]:].any()               # exactly 0 past the length
        if n[b] == 0:
            assert host(loss)[b] == 0              # and the loss of an empty row is exactly 0


# ------------------------------------------------------------------------------------------------- narrow kernel

@pytest.mark.parametrize('e', [0.1, 0.5])
@pytest.mark.parametrize('C', [1, 2, 9, 41, 1023])
def test_narrow_kernel(C, e):
    logits, targets, ll, tl = _case(C)
    loss, dl, clean = _raw(False, dev(logits), dev(targets), dev(ll), dev(tl), e)
    assert clean
    _check(loss, dl, logits, targets, ll, tl, e)
    l2, d2 = hip.xent_smooth_loss_grad(dev(logits), dev(targets), dev(ll), dev(tl), SCALE, e)      # the wrapper
    assert torch.equal(l2, loss) and torch.equal(d2, dl)


def test_narrow_kernel_second_frame_of_a_thread():
    """L = 300 > 256 threads: threads 0..43 take a second frame"""
    ll = np.array([300, 257, 256, 1, 0], np.int32)
    tl = np.array([300, 260, 256, 1, 3], np.int32)
    logits, targets, _, _ = _case(41, L_=300, seed=300)
    loss, dl, clean = _raw(False, dev(logits), dev(targets), dev(ll), dev(tl), 0.1)
    assert clean
    _check(loss, dl, logits, targets, ll, tl, 0.1)


# ------------------------------------------------------------------------------------------------- wide kernel

@pytest.mark.parametrize('C', [1024, 1031, 3100])
def test_wide_kernel(C):
    e = 0.1
    logits, targets, ll, tl = _case(C)
    lg = dev(logits)
    assert lg.data_ptr() % 16 == 0
    loss, dl, clean = _raw(True, lg, dev(targets), dev(ll), dev(tl), e)             # aligned: the float4 body
    assert clean
    _check(loss, dl, logits, targets, ll, tl, e)
    loss2, dl2, _ = _raw(True, lg, dev(targets), dev(ll), dev(tl), e)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)                        # deterministic
    l2, d2 = hip.xent_wide_smooth_loss_grad(lg, dev(targets), dev(ll), dev(tl), SCALE, e)         # the wrapper
    assert torch.equal(l2, loss) and torch.equal(d2, dl)
    # one float off the 16-byte phase, logits and dlogits alike: scalar head, float4 body, scalar tail
    buf = torch.zeros(B * L * C + 1, device='cuda')
    v = buf[1:].view(B, L, C)
    v.copy_(lg)
    loss3, dl3, clean = _raw(True, v, dev(targets), dev(ll), dev(tl), e, phase=1)
    assert clean
    _check(loss3, dl3, logits, targets, ll, tl, e)
    # and against an aligned dlogits the phases differ: all scalar
    loss4, dl4, clean = _raw(True, v, dev(targets), dev(ll), dev(tl), e, phase=0)
    assert clean
    _check(loss4, dl4, logits, targets, ll, tl, e)
    if C == 1024:                                  # the routing threshold: both kernels agree
        l0, d0, _ = _raw(False, lg, dev(targets), dev(ll), dev(tl), e)
        assert rel(host(loss), host(l0).astype(np.float64)) <= LOSS_BAR
        assert rel(host(dl), host(d0).astype(np.float64)) <= GRAD_BAR


# ------------------------------------------------------------------------------------------------- smoothing = 0

@pytest.mark.parametrize('C', [41, 1031])
def test_zero_smoothing_is_bit_identical_to_the_plain_entry_points(C):
    logits, targets, ll, tl = _case(C)
    wide = C >= loss_functions.WIDE_XENT_MIN_CLASSES
    plain = hip.xent_wide_loss_grad if wide else hip.xent_loss_grad
    smooth = hip.xent_wide_smooth_loss_grad if wide else hip.xent_smooth_loss_grad
    l0, d0 = plain(dev(logits), dev(targets), dev(ll), dev(tl), SCALE)
    l1, d1 = smooth(dev(logits), dev(targets), dev(ll), dev(tl), SCALE, 0.0)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)
    l2, d2, clean = _raw(wide, dev(logits), dev(targets), dev(ll), dev(tl), 0.0)
    assert clean and torch.equal(l0, l2) and torch.equal(d0, d2)
    # and smoothing does something
    l3, _ = smooth(dev(logits), dev(targets), dev(ll), dev(tl), SCALE, 0.1)
    assert not torch.equal(l0, l3)


# ------------------------------------------------------------------------------------------------- saturation

@pytest.mark.parametrize('C', [41, 1031])
@pytest.mark.parametrize('on', [True, False])
def test_saturated_and_equal_logits(C, on):
    """one logit at +80 and the rest at -80, the label on the large logit or off it; then all logits equal, where
    loss_t = log C and d_c = s * (1/C - q_c) whatever the smoothing"""
    rng = np.random.default_rng(C)
    wide = C >= loss_functions.WIDE_XENT_MIN_CLASSES
    big = rng.integers(0, C, (B, L))
    logits = np.full((B, L, C), -80.0, np.float32)
    np.put_along_axis(logits, big[:, :, None], 80.0, 2)
    targets = np.zeros((B, L + 2), np.int32)
    targets[:, :L] = big if on else (big + 1 + rng.integers(0, C - 1, (B, L))) % C
    for e in (0.1, 0.5):
        loss, dl, clean = _raw(wide, dev(logits), dev(targets), dev(LOGIT_LEN), dev(TARGET_LEN), e)
        assert clean and torch.isfinite(loss).all() and torch.isfinite(dl).all()
        _check(loss, dl, logits, targets, LOGIT_LEN, TARGET_LEN, e)
        flat = np.full((B, L, C), 1.75, np.float32)
        loss, dl, clean = _raw(wide, dev(flat), dev(targets), dev(LOGIT_LEN), dev(TARGET_LEN), e)
        assert clean
        _check(loss, dl, flat, targets, LOGIT_LEN, TARGET_LEN, e)
        assert rel(host(loss), LOGIT_LEN * np.log(C) / TARGET_LEN) <= LOSS_BAR
        q = np.full((B, L, C), e / C)
        np.put_along_axis(q, targets[:, :L, None].astype(np.int64), 1 - e + e / C, 2)
        live = np.arange(L)[None, :] < LOGIT_LEN[:, None]
        want = (SCALE / TARGET_LEN)[:, None, None] * (1.0 / C - q) * live[:, :, None]
        assert rel(host(dl), want) <= GRAD_BAR


# ------------------------------------------------------------------------------------------------- loss functions

def _trainer(recipe, data, **over):
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0)


CFG3 = {'encoder.num_units': 16, 'decoder.num_units': 16, 'encoder.gemm_precision': 'f32', 'encoder.dropout': 1,
        'encoder.input_noise': 0, 'decoder.dropout': 1, 'decoder.sample_prob': 0, 'trainer.batch_size': 4}


def _cfg3_data(num_labels=39, seed=3234, batches=100):
    return SyntheticData(4, 32, 40, num_labels=num_labels, min_frames=20, min_labels=2, max_labels=5, eos=True,
                         time_reduction=8, seed=seed, batches_per_epoch=batches)


def _model_logits(recipe, data, name, **over):
    """the logits, logit lengths, targets and target lengths of batch 0 under the model's initial weights"""
    tr = _trainer(recipe, data, **over)
    raw = data.batch(0)
    b = tr.to_device(raw)
    with torch.no_grad():
        logits, lsl = tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)
    torch.cuda.synchronize()
    return logits[name], lsl[name], raw['targets'][name], raw['target_seq_length'][name]


def _loss_and_tape_gradients(name, e, outputs):
    """factory(name, label_smoothing=e) over `outputs` {output: (logits, logit_len, targets, target_len)}: the loss
    and, per output, the gradient the tape hands to whatever produced the logits"""
    got, srcs = {}, {}
    with Tape() as tape:
        for o, (lg, _, _, _) in outputs.items():
            srcs[o] = lg.clone()

            def capture(g, o=o):
                got[o] = g
                return [None]
            record([srcs[o]], [lg], capture)       # makes the logits an interior node of the tape
        loss = loss_functions.factory(name, label_smoothing=e)(
            {o: dev(v[2]) for o, v in outputs.items()}, {o: v[0] for o, v in outputs.items()},
            {o: SeqLen.wrap(v[1], 'cuda') for o, v in outputs.items()}, {o: SeqLen(v[3], 'cuda') for o, v in outputs.items()})
    tape.backward(loss)
    torch.cuda.synchronize()
    return float(loss.item()), got


def _reference(name, e, outputs):
    total, grads = 0.0, {}
    for o, (lg, ll, tg, tl) in outputs.items():
        x = host(lg)
        n = SeqLen.wrap(ll, 'cuda').host
        if name == 'average_cross_entropy':
            per, g = R.average(x, tg, n, tl, e, grad_scale=1.0 / x.shape[0])
        else:
            per, g = R.summed(x, tg, tl, e, grad_scale=1.0 / x.shape[0])
        total += per.mean()
        grads[o] = g
    return total, grads


@pytest.fixture(scope='module')
def las_outputs():
    """the Speller decodes its first output only (as the reference's does), so the two outputs of different class
    counts are the logits of two shrunken cfg3 models: 39 + eos and 23 + eos classes"""
    return {'text': _model_logits('cfg3_las_vanilla', _cfg3_data(39, 3234), 'text', **CFG3),
            'other': _model_logits('cfg3_las_vanilla', _cfg3_data(23, 3235), 'text',
                                   **dict(CFG3, **{'io.output_dims': 23}))}


@pytest.fixture(scope='module')
def dnn_outputs():
    data = SyntheticData(3, 24, 13, num_labels=1100, min_frames=9, frame_targets=True, target_name='alignments', seed=7)
    over = {'encoder.context': 2, 'encoder.num_units': 32, 'encoder.num_layers': 2, 'encoder.dropout': 1,
            'encoder.gemm_precision': 'f32', 'io.output_dims': 1100, 'trainer.batch_size': 3}
    return {'alignments': _model_logits('dnn_hybrid_wsj', data, 'alignments', **over)}


@pytest.mark.parametrize('name', ['average_cross_entropy', 'sum_cross_entropy'])
@pytest.mark.parametrize('model', ['las', 'dnn'])
def test_loss_functions_on_a_models_logits(model, name, las_outputs, dnn_outputs):
    outputs = las_outputs if model == 'las' else dnn_outputs
    classes = sorted(v[0].shape[2] for v in outputs.values())
    assert classes == ([24, 40] if model == 'las' else [1100])
    loss, grads = _loss_and_tape_gradients(name, 0.1, outputs)
    want, wgrads = _reference(name, 0.1, outputs)
    print(model, name, 'loss', loss, 'reference', want)
    assert abs(loss - want) / abs(want) <= 1e-6
    for o in outputs:
        assert rel(host(grads[o]), wgrads[o]) <= 1e-5, o
    # and the smoothing is seen: without it the gradients are somewhere else (the losses hardly differ on the nearly
    # uniform softmax of an untrained model, where every target costs about log C)
    _, pgrads = _loss_and_tape_gradients(name, 0.0, outputs)
    for o in outputs:
        assert rel(host(pgrads[o]), wgrads[o]) > 1e-2, o


def test_without_smoothing_the_factory_calls_the_plain_wrappers(monkeypatch, las_outputs, dnn_outputs):
    """a run without the key takes the code path it always took: hip.xent_loss_grad / hip.xent_wide_loss_grad"""
    counts = {}

    def counted(fname):
        fn = getattr(hip, fname)

        def wrapper(*a):
            counts[fname] = counts.get(fname, 0) + 1
            return fn(*a)
        monkeypatch.setattr(hip, fname, wrapper)
    for fname in ('xent_loss_grad', 'xent_wide_loss_grad', 'xent_smooth_loss_grad', 'xent_wide_smooth_loss_grad'):
        counted(fname)
    for name in ('average_cross_entropy', 'sum_cross_entropy'):
        counts.clear()
        _loss_and_tape_gradients(name, 0.0, las_outputs)
        _loss_and_tape_gradients(name, 0.0, dnn_outputs)
        assert counts == {'xent_loss_grad': 2, 'xent_wide_loss_grad': 1}
        counts.clear()
        _loss_and_tape_gradients(name, 0.1, las_outputs)
        _loss_and_tape_gradients(name, 0.1, dnn_outputs)
        assert counts == {'xent_smooth_loss_grad': 2, 'xent_wide_smooth_loss_grad': 1}


# ------------------------------------------------------------------------------------------------- trainer

class OneBatch(object):
    """a batch source that serves batch 0 of `data` at every step"""

    def __init__(self, data, steps):
        self.data, self.steps = data, steps

    def num_batches(self):
        return self.steps

    def batch(self, step):
        return self.data.batch(0)

    def validation(self, numbatches, batch_size=None):
        return self.data.validation(numbatches, batch_size)


def test_trainer_one_step():
    data = _cfg3_data()
    over = dict(CFG3, **{'evaluator.batch_size': 2, 'evaluator.numbatches': 2})
    plain = _trainer('cfg3_las_vanilla', data, **over)
    smooth = _trainer('cfg3_las_vanilla', data, **dict(over, **{'trainer.label_smoothing': 0.1}))
    raw = data.batch(0)
    # identical initial weights: the validation loss is the same number under both confs
    for tr in (plain, smooth):
        tr._create_graph()
        tr._ensure_variables()
    a, b = plain.model.store.state_dict(), smooth.model.store.state_dict()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert plain.validation_loss() == smooth.validation_loss()
    # the two losses differ by the reference's difference on that batch's logits
    bd = plain.to_device(raw)
    with torch.no_grad():
        logits, lsl = plain.model(bd['inputs'], bd['input_seq_length'], bd['targets'], bd['target_seq_length'], True)
    outputs = {'text': (logits['text'], lsl['text'], raw['targets']['text'], raw['target_seq_length']['text'])}
    r0, _ = _reference('average_cross_entropy', 0.0, outputs)
    r1, _ = _reference('average_cross_entropy', 0.1, outputs)
    l0 = float(plain.step(plain.to_device(raw)).item())
    l1 = float(smooth.step(smooth.to_device(raw)).item())
    print('losses', l0, l1, 'reference', r0, r1)
    # each loss within the kernels' bar of its reference, hence their difference within twice that of the reference's
    # (which is small on an untrained model's nearly uniform softmax, and still some hundred times the bar)
    assert abs(l0 - r0) <= LOSS_BAR * r0 and abs(l1 - r1) <= LOSS_BAR * r1
    assert abs((l1 - l0) - (r1 - r0)) <= 2 * LOSS_BAR * r1 and abs(r1 - r0) > 50 * LOSS_BAR * r1
    torch.cuda.synchronize()
    a, b = plain.model.store.state_dict(), smooth.model.store.state_dict()
    assert any(not np.array_equal(a[k], b[k]) for k in a)
    # on identical weights the validation loss is again the same number
    smooth.load_state(plain.state())
    assert plain.validation_loss() == smooth.validation_loss()


@pytest.fixture(scope='module')
def thirty_steps():
    def run(prefetch):
        data = OneBatch(_cfg3_data(), 30)
        over = dict(CFG3, **{'trainer.label_smoothing': 0.1, 'trainer.num_epochs': 1, 'evaluator.evaluator': 'None'})
        if prefetch:
            over['trainer.prefetch_batches'] = prefetch
        tr = _trainer('cfg3_las_vanilla', data, **over)
        return tr, tr.train()
    return run


def test_trainer_repeated_steps_on_one_batch(thirty_steps):
    tr, hist = thirty_steps(0)
    losses = np.array([h[1] for h in hist])
    assert len(losses) == 30 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    raw = tr.data.batch(0)
    b = tr.to_device(raw)
    with torch.no_grad():
        logits, lsl = tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)
    C = logits['text'].shape[2]
    assert C == 40                                 # the model's output dimension: eos counts
    n = np.minimum(SeqLen.wrap(lsl['text'], 'cuda').host, logits['text'].shape[1])
    floor = float(np.mean(n * R.entropy(C, 0.1) / raw['target_seq_length']['text']))
    print('first %.6f last %.6f floor %.6f' % (losses[0], losses[-1], floor))
    assert floor > 0.4 and (losses >= floor).all()
    _, overlapped = thirty_steps(2)
    assert overlapped == hist
