"""CPU: the float64 reference of the label-smoothed cross-entropy (tests/xent_smooth_ref.py) against torch and in
closed form, the host-side argument checks of the two new entry points, the loss factory and the trainer key."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from nabu_amd import recipes
from nabu_amd.processing.synthetic import SyntheticData
from tests import torch_ref
from tests import xent_smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, L, C = 5, 19, 9
LOGIT_LEN = np.array([19, 4, 11, 1, 0], np.int32)
TARGET_LEN = np.array([19, 4, 11, 1, 3], np.int32)


def _case(seed=0, classes=C):
    rng = np.random.default_rng(seed)
    return 3 * rng.standard_normal((B, L, classes)), rng.integers(0, classes, (B, L + 2)).astype(np.int32)


def _torch_formula(logits, targets, mask_len, divisor, e):
    """autograd of the written-out formula: (loss [B], d sum_b loss[b] / d logits)"""
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(targets[:, :L].astype(np.int64))
    lz = torch.logsumexp(x, -1)
    frame = lz - (1 - e) * x.gather(2, y[:, :, None])[:, :, 0] - e * x.mean(-1)
    live = torch.arange(L)[None, :] < torch.tensor(mask_len.astype(np.int64))[:, None]
    loss = (frame * live).sum(1) / torch.tensor(np.asarray(divisor, np.float64))
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize('e', [0.0, 0.1, 0.125, 0.5])
def test_reference_equals_autograd_of_the_formula_under_both_masks(e):
    logits, targets = _case(1)
    for got, want in ((R.average(logits, targets, LOGIT_LEN, TARGET_LEN, e),
                       _torch_formula(logits, targets, LOGIT_LEN, TARGET_LEN, e)),
                      (R.summed(logits, targets, TARGET_LEN, e),
                       _torch_formula(logits, targets, TARGET_LEN, np.ones(B), e))):
        assert np.abs(got[0] - want[0]).max() <= 1e-12
        assert np.abs(got[1] - want[1]).max() <= 1e-12
    # grad_scale scales the gradient and nothing else
    l2, d2 = R.average(logits, targets, LOGIT_LEN, TARGET_LEN, e, grad_scale=0.2)
    l1, d1 = R.average(logits, targets, LOGIT_LEN, TARGET_LEN, e)
    assert np.array_equal(l1, l2) and np.abs(d2 - 0.2 * d1).max() <= 1e-15
    assert l1[4] == 0 and not d1[4].any() and not d1[1, 4:].any()


def test_reference_equals_torch_cross_entropy_at_a_smoothing_exact_in_single_precision():
    """0.125 is the same number in single and double precision, so the comparison does not depend on the precision
    in which torch holds its label_smoothing constant"""
    F = torch.nn.functional
    logits, targets = _case(2)
    ones = np.ones(B)

    def torch_ce(e):
        x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        y = torch.tensor(targets[:, :L].astype(np.int64))
        ce = F.cross_entropy(x.reshape(B * L, C), y.reshape(-1), reduction='none', label_smoothing=e).reshape(B, L)
        ce.sum().backward()
        return ce.detach().numpy(), x.grad.numpy()
    ce, g = torch_ce(0.125)
    loss, d = R.per_utterance(logits, targets, np.full(B, L), ones, 0.125)
    assert np.abs(loss - ce.sum(1)).max() <= 1e-12
    assert np.abs(d - g).max() <= 1e-12


def test_reference_without_smoothing_is_the_plain_loss():
    logits, targets = _case(3)
    lens = np.array([19, 4, 11, 1, 7], np.int32)
    loss, _ = R.average(logits, targets, lens, TARGET_LEN, 0.0)
    want = torch_ref.avg_xent(torch.tensor(logits), targets, lens, TARGET_LEN)
    assert abs(loss.mean() - float(want)) <= 1e-12


@pytest.mark.parametrize('classes', [1, 2, 9, 1031])
@pytest.mark.parametrize('e', [0.0, 0.1, 0.5])
def test_closed_form_for_equal_logits(classes, e):
    """all logits equal: softmax is uniform, so loss_t = log C whatever e is and d_c = s * (1/C - q_c)"""
    rng = np.random.default_rng(classes)
    logits = np.full((B, L, classes), 1.75)
    targets = rng.integers(0, classes, (B, L)).astype(np.int32)
    loss, d = R.average(logits, targets, LOGIT_LEN, TARGET_LEN, e, grad_scale=0.2)
    assert np.abs(loss - LOGIT_LEN * math.log(classes) / TARGET_LEN).max() <= 1e-12
    q = np.full((B, L, classes), e / classes)
    np.put_along_axis(q, targets[:, :, None].astype(np.int64), 1 - e + e / classes, 2)
    live = np.arange(L)[None, :] < LOGIT_LEN[:, None]
    want = (0.2 / TARGET_LEN)[:, None, None] * (1.0 / classes - q) * live[:, :, None]
    assert np.abs(d - want).max() <= 1e-15
    # and the entropy of q is the floor of a frame's loss: reached by logits = log q
    if e > 0:
        lq = np.log(q)
        floor, _ = R.per_utterance(lq, targets, np.full(B, L), np.ones(B), e)
        assert np.abs(floor - L * R.entropy(classes, e)).max() <= 1e-9
        assert (loss * TARGET_LEN >= LOGIT_LEN * R.entropy(classes, e) - 1e-12).all()


# ------------------------------------------------------------------------------------------------- C ABI

def _lib():
    from nabu_amd import _hip, build
    build.build(verbose=False)
    return _hip.lib()


P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(7)]       # never touched: every refusal precedes the launch


def _narrow(lib, smoothing, ptrs=P):
    lg, tg, ll, tl, loss, dl = ptrs[:6]
    return lib.nabu_xent_smooth_loss_grad(2, 4, 3, 4, lg, tg, ll, tl, 1.0, smoothing, loss, dl, None)


def _wide(lib, smoothing, ptrs=P, ws_bytes=2 * 4 * 4):
    lg, tg, ll, tl, loss, dl, ws = ptrs
    return lib.nabu_xent_wide_smooth_loss_grad(2, 4, 3, 4, lg, tg, ll, tl, 1.0, smoothing, loss, dl, ws, ws_bytes, None)


def test_symbols_declared_bound_and_wrapped():
    from nabu_amd import _hip, ops
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'nabu_hip.h')).read()
    for name in ('nabu_xent_smooth_loss_grad', 'nabu_xent_wide_smooth_loss_grad'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(lib, name)
        plain = _hip.SIGNATURES[name.replace('_smooth', '')][1]
        assert _hip.SIGNATURES[name][1] == plain[:9] + [ctypes.c_float] + plain[9:]      # one float after grad_scale
    assert callable(ops.xent_smooth_loss_grad) and callable(ops.xent_wide_smooth_loss_grad)
    assert lib.nabu_version() == _hip.ABI_VERSION == 4


@pytest.mark.parametrize('call', [_narrow, _wide])
@pytest.mark.parametrize('smoothing', [-0.1, 1.0, float('nan')])
def test_smoothing_outside_its_range_is_refused_on_the_host(call, smoothing):
    lib = _lib()
    assert call(lib, smoothing) == -1
    assert b'smoothing' in lib.nabu_last_error(), lib.nabu_last_error()


@pytest.mark.parametrize('call', [_narrow, _wide])
def test_null_pointers_and_bad_dimensions_fail_as_the_plain_entry_points_do(call):
    lib = _lib()
    for i in range(6 if call is _narrow else 7):
        ptrs = list(P)
        ptrs[i] = None
        assert call(lib, 0.1, ptrs) == -1
        assert b'null' in lib.nabu_last_error(), (i, lib.nabu_last_error())
    lg, tg, ll, tl, loss, dl, ws = P
    assert lib.nabu_xent_smooth_loss_grad(2, 4, 0, 4, lg, tg, ll, tl, 1.0, 0.1, loss, dl, None) == -1
    assert lib.nabu_xent_smooth_loss_grad(2, 4, 3, 3, lg, tg, ll, tl, 1.0, 0.1, loss, dl, None) == -1       # ldt < L
    assert lib.nabu_xent_wide_smooth_loss_grad(0, 4, 3, 4, lg, tg, ll, tl, 1.0, 0.1, loss, dl, ws, 64, None) == -1
    assert b'dimensions' in lib.nabu_last_error()


def test_wide_entry_refuses_a_short_workspace():
    lib = _lib()
    need = lib.nabu_xent_wide_ws_bytes(2, 4)
    assert need == 2 * 4 * 4
    assert _wide(lib, 0.1, ws_bytes=need - 1) == -3
    assert b'workspace' in lib.nabu_last_error()


# ------------------------------------------------------------------------------------------------- factory, trainer

def test_factory_binds_the_smoothing_into_the_cross_entropy_losses_only():
    from nabu_amd.neuralnetworks.trainers import loss_functions as lf
    assert lf.factory('average_cross_entropy') is lf.average_cross_entropy
    assert lf.factory('sum_cross_entropy', label_smoothing=0.0) is lf.sum_cross_entropy
    for name in ('average_cross_entropy', 'sum_cross_entropy'):
        fn = lf.factory(name, label_smoothing=0.1)
        assert callable(fn) and fn.keywords == {'label_smoothing': 0.1} and fn.func is getattr(lf, name)
    assert lf.factory('CTC') is lf.CTC and lf.factory('CTC', label_smoothing=0.0) is lf.CTC
    with pytest.raises(ValueError, match='cross-entropy losses only'):
        lf.factory('CTC', label_smoothing=0.1)
    for bad in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError, match='label_smoothing'):
            lf.factory('average_cross_entropy', label_smoothing=bad)


def test_without_smoothing_the_losses_call_the_entry_points_they_always_called(monkeypatch):
    """a run without the key: factory(name) reaches hip.xent_loss_grad / hip.xent_wide_loss_grad with the same
    arguments, and never the smoothing wrappers; with the key it is the other way round"""
    from nabu_amd import ops as hip
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.trainers import loss_functions as lf
    calls = []

    def fake(name):
        def fn(logits, targets, ll, tl, scale, *smoothing):
            calls.append((name, tuple(logits.shape), scale) + smoothing)
            return torch.zeros(logits.shape[0]), torch.zeros_like(logits)
        return fn
    for name in ('xent_loss_grad', 'xent_wide_loss_grad', 'xent_smooth_loss_grad', 'xent_wide_smooth_loss_grad'):
        monkeypatch.setattr(hip, name, fake(name))
    monkeypatch.setattr(hip, 'sum_', lambda x, scale=1.0: (x.sum() * scale).reshape(1))
    monkeypatch.setattr(hip, 'axpy_', lambda y, x, a=1.0: y.add_(a * x))
    lens = SeqLen([3, 2], dev_tensor=torch.tensor([3, 2], dtype=torch.int32))
    logits = {'text': torch.zeros(2, 3, 40), 'states': torch.zeros(2, 3, lf.WIDE_XENT_MIN_CLASSES)}
    targets = {k: torch.zeros(2, 3, dtype=torch.int32) for k in logits}
    sl = {k: lens for k in logits}
    for loss in ('average_cross_entropy', 'sum_cross_entropy'):
        del calls[:]
        lf.factory(loss)(targets, logits, sl, sl)
        assert calls == [('xent_loss_grad', (2, 3, 40), 0.5), ('xent_wide_loss_grad', (2, 3, 1024), 0.5)]
        del calls[:]
        lf.factory(loss, label_smoothing=0.0)(targets, logits, sl, sl)
        assert [c[0] for c in calls] == ['xent_loss_grad', 'xent_wide_loss_grad']
        del calls[:]
        lf.factory(loss, label_smoothing=0.1)(targets, logits, sl, sl)
        assert calls == [('xent_smooth_loss_grad', (2, 3, 40), 0.5, 0.1),
                         ('xent_wide_smooth_loss_grad', (2, 3, 1024), 0.5, 0.1)]


def _trainer(recipe='cfg3_las_vanilla', **over):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(4, 32, 40), modelconf=mc,
                                               evaluatorconf=ec, expdir=None, server=None, task_index=0)


@pytest.mark.parametrize('value', ['abc', '-0.1', '1', 'nan'])
def test_trainer_refuses_a_bad_key_naming_it(value):
    with pytest.raises(ValueError, match='label_smoothing'):
        _trainer(**{'trainer.label_smoothing': value})


def test_trainer_refuses_smoothing_with_ctc_at_construction():
    with pytest.raises(ValueError, match='cross-entropy losses only'):
        _trainer('cfg2_listener_ctc', **{'trainer.label_smoothing': 0.1})
    assert _trainer('cfg2_listener_ctc', **{'trainer.label_smoothing': 0}).label_smoothing == 0.0


def test_trainer_reads_the_key_and_a_conf_without_it_builds_as_before():
    tr = _trainer()
    assert 'label_smoothing' not in tr.conf and tr.label_smoothing == 0.0
    tr = _trainer(**{'trainer.label_smoothing': 0.1})
    assert tr.label_smoothing == 0.1


def test_no_shipped_recipe_or_defaults_file_sets_the_key():
    for recipe in sorted(os.listdir(recipes.RECIPES)):
        if os.path.isdir(os.path.join(recipes.RECIPES, recipe)):
            _, tc, ec = recipes.load_recipe(recipe)
            assert not tc.has_option('trainer', 'label_smoothing'), recipe
            assert not ec.has_option('evaluator', 'label_smoothing'), recipe
    for sub in ('trainers', 'evaluators'):
        d = os.path.join(ROOT, 'nabu_amd', 'neuralnetworks', sub, 'defaults')
        for name in os.listdir(d):
            assert not re.search(r'^\s*label_smoothing\s*=', open(os.path.join(d, name)).read(), flags=re.M), name


def test_the_evaluator_asks_for_the_unsmoothed_loss(monkeypatch):
    """LossEvaluator.update_loss calls factory(conf['loss']) and nothing else: validation is not smoothed"""
    import inspect
    from nabu_amd.neuralnetworks.evaluators import loss_evaluator
    src = inspect.getsource(loss_evaluator.LossEvaluator.update_loss)
    assert "loss_functions.factory(self.conf['loss'])(" in src
    assert 'never label-smoothed' in loss_evaluator.__doc__
