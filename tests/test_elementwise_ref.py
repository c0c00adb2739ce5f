"""CPU: the float64 restatements behind tests/test_hip_elementwise.py against torch autograd in float64 — the LSTM cell's
backward pass (tests/elementwise_ref.py) and the oracle's whole-utterance layer_norm_bwd — and the rules a formula
cannot be differentiated for: frozen rows, NaN through clip, the shape of the sum."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from tests import elementwise_ref as R

B, U, C = 6, 5, 4
SEQ_LEN = np.array([3, 0, 2, 7, 1, 3], np.int32)       # at step 2: rows 0, 3, 5 live; 1, 2, 4 finished


def _cell_case(seed=0):
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s)
    return dict(z=n(B, 4 * U), bias=n(4 * U), c_prev=n(B, U), h_prev=n(B, U), emb=n(C, 4 * U),
                ids=rng.integers(0, C, B).astype(np.int32), dh=n(B, U), dh2=n(B, U), dc_in=n(B, U))


def _torch_cell(k, with_emb, with_dh2, live):
    """autograd of the written-out cell: d (sum(h' (dh + dh2)) + sum(c' dc_in)) / d z and / d c_prev"""
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    z = t(k['z']).requires_grad_(True)
    c_prev = t(k['c_prev']).requires_grad_(True)
    zz = z + t(k['bias'])
    if with_emb:
        zz = zz + t(k['emb'])[torch.tensor(k['ids'].astype(np.int64))]
    i, g = torch.sigmoid(zz[:, :U]), torch.tanh(zz[:, U:2 * U])
    f, o = torch.sigmoid(zz[:, 2 * U:3 * U] + 1.0), torch.sigmoid(zz[:, 3 * U:])
    c = c_prev * f + i * g
    h = torch.tanh(c) * o
    dht = t(k['dh']) + (t(k['dh2']) if with_dh2 else 0.0)
    m = t(live.astype(np.float64))[:, None]
    ((h * dht * m).sum() + (c * t(k['dc_in']) * m).sum()).backward()
    return (torch.cat([i, g, f, o], 1).detach().numpy(), c.detach().numpy(), h.detach().numpy(), z.grad.numpy(),
            c_prev.grad.numpy())


@pytest.mark.parametrize('with_dh2', [False, True])
@pytest.mark.parametrize('with_emb', [False, True])
def test_cell_restatement_equals_autograd_on_live_rows_and_freezes_the_others(with_emb, with_dh2):
    k = _cell_case(1)
    step = 2
    live = step < SEQ_LEN
    assert live.tolist() == [True, False, False, True, False, True]
    emb, ids = (k['emb'], k['ids']) if with_emb else (None, None)
    acts, c_new, h_new = R.lstm_cell_fwd(step, SEQ_LEN, k['z'], k['bias'], k['c_prev'], k['h_prev'], emb, ids)
    dz, dc_out = R.lstm_cell_bwd(step, SEQ_LEN, acts, c_new, k['c_prev'], k['dh'], k['dc_in'],
                                 k['dh2'] if with_dh2 else None)
    ta, tc, th, tdz, tdc = _torch_cell(k, with_emb, with_dh2, live)
    for got, want in ((acts, ta), (c_new, tc), (h_new, th), (dz, tdz), (dc_out, tdc)):
        assert np.abs(got[live] - want[live]).max() <= 1e-14
    # finished rows: the state is copied, activations and dz are zero, dc passes through — exactly
    dead = ~live
    assert np.array_equal(c_new[dead], k['c_prev'][dead]) and np.array_equal(h_new[dead], k['h_prev'][dead])
    assert not acts[dead].any() and not dz[dead].any()
    assert np.array_equal(dc_out[dead], k['dc_in'][dead])
    # the one-hot row and the second dh change something
    if with_emb:
        assert np.abs(acts - R.lstm_cell_fwd(step, SEQ_LEN, k['z'], k['bias'], k['c_prev'], k['h_prev'])[0]).max() > 1e-3
    if with_dh2:
        assert np.abs(dz - R.lstm_cell_bwd(step, SEQ_LEN, acts, c_new, k['c_prev'], k['dh'], k['dc_in'])[0]).max() > 1e-3


@pytest.mark.parametrize('step,live', [(0, [1, 0, 1, 1, 1, 1]), (1, [1, 0, 1, 1, 0, 1]), (3, [0, 0, 0, 1, 0, 0]),
                                       (7, [0, 0, 0, 0, 0, 0])])
def test_cell_freezes_a_row_from_the_step_that_equals_its_length(step, live):
    k = _cell_case(2)
    live = np.array(live, bool)
    acts, c_new, h_new = R.lstm_cell_fwd(step, SEQ_LEN, k['z'], k['bias'], k['c_prev'], k['h_prev'])
    dz, dc_out = R.lstm_cell_bwd(step, SEQ_LEN, acts, c_new, k['c_prev'], k['dh'], k['dc_in'])
    assert np.array_equal(acts.any(1), live) and np.array_equal(dz.any(1), live)
    assert np.array_equal((c_new != k['c_prev']).any(1), live) and np.array_equal((h_new != k['h_prev']).any(1), live)
    assert np.array_equal((dc_out != k['dc_in']).any(1), live)


def test_cell_in_single_precision_is_single_precision_and_close():
    k = _cell_case(3)
    a64 = R.lstm_cell_fwd(0, SEQ_LEN, k['z'], k['bias'], k['c_prev'], k['h_prev'], k['emb'], k['ids'])
    a32 = R.lstm_cell_fwd(0, SEQ_LEN, k['z'], k['bias'], k['c_prev'], k['h_prev'], k['emb'], k['ids'], np.float32)
    b32 = R.lstm_cell_bwd(0, SEQ_LEN, a32[0], a32[1], k['c_prev'], k['dh'], k['dc_in'], k['dh2'], np.float32)
    for x32 in a32 + b32:
        assert x32.dtype == np.float32
    for x32, x64 in zip(a32, a64):
        assert x64.dtype == np.float64 and 0 < np.abs(x32 - x64).max() < 1e-5


def test_cell_gates_saturate_to_exact_limits_without_nan():
    z = np.array([[-800., 800., 800., -800.], [800., -800., -800., 800.]])
    acts, c, h = R.lstm_cell_fwd(0, [1, 1], z, np.zeros(4), np.ones((2, 1)), np.ones((2, 1)), dtype=np.float32)
    assert acts.tolist() == [[0., 1., 1., 0.], [1., -1., 0., 1.]]
    assert c.tolist() == [[1.], [-1.]] and h[0, 0] == 0 and abs(h[1, 0] - np.tanh(-1.0)) < 1e-7


@pytest.mark.parametrize('shape', [(1, 1, 4), (3, 7, 10), (2, 30, 8)])
def test_oracle_layer_norm_bwd_equals_autograd(shape):
    rng = np.random.default_rng(shape[1])
    Bn, F = shape[0], shape[-1]
    x, dy = rng.standard_normal(shape) + 3.0, rng.standard_normal(shape)
    gamma, beta = rng.standard_normal(F) + 1.0, rng.standard_normal(F)
    eps = 1e-3 if shape == (1, 1, 4) else 1e-12
    y, cache = O.layer_norm_fwd(x, gamma, beta, eps)
    dx, dgamma, dbeta = O.layer_norm_bwd(dy, cache)
    tx, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, gamma, beta))
    flat = tx.reshape(Bn, -1)
    mu = flat.mean(1).reshape(Bn, 1, 1)
    var = ((flat - flat.mean(1, keepdim=True)) ** 2).mean(1).reshape(Bn, 1, 1)
    ty = (tx - mu) / torch.sqrt(var + eps) * tg + tb
    (ty * torch.tensor(dy)).sum().backward()
    scale = max(1.0, float(np.abs(cache[1]).max()))
    assert np.abs(y - ty.detach().numpy()).max() <= 1e-12 * scale
    assert np.abs(dx - tx.grad.numpy()).max() <= 1e-11 * scale
    assert np.abs(dgamma - tg.grad.numpy()).max() <= 1e-11 * scale
    assert np.abs(dbeta - tb.grad.numpy()).max() <= 1e-12


def test_clip_keeps_nan_and_bounds_everything_else():
    x = np.array([np.nan, -np.inf, np.inf, -0.0, 0.3, -0.3, 0.25, 1e-45], np.float32)
    for dtype in (np.float32, np.float64):
        y = R.clip(x, 0.25, dtype)
        assert y.dtype == dtype and np.isnan(y[0])
        assert y[1:].tolist() == [-0.25, 0.25, -0.0, 0.25, -0.25, 0.25, dtype(x[7])]
        assert np.signbit(y[3])
    assert np.array_equal(R.clip(x, 0.25, np.float32)[1:], np.clip(x, -0.25, 0.25)[1:])


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 1000])
def test_sum_tree_is_the_sum_in_double_and_within_its_bound_in_single(n):
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    s64 = R.sum_tree(x, 0.5)
    assert abs(s64 - 0.5 * x.astype(np.float64).sum()) <= 1e-13 * max(1.0, np.abs(x).sum())
    s32 = R.sum_tree(x, 0.5, np.float32)
    assert isinstance(s32, np.float32)
    assert abs(float(s32) - s64) <= (-(-n // 256) + 8) * 2.0 ** -24 * 0.5 * np.abs(x.astype(np.float64)).sum()
    if n == 0:
        assert s32 == 0 and s64 == 0


def test_sum_tree_adds_in_chains_of_stride_256():
    """2^24 + 1 + 1 loses both ones when they are added one at a time to the large number (one chain), not when they
    sit in other chains and meet each other first in the tree"""
    x = np.zeros(512, np.float32)
    x[0], x[256], x[1], x[3] = 2.0 ** 24, 1.0, 1.0, 1.0
    # chain 0: 2^24 + 1 -> 2^24 (lost); chains 1 and 3 hold a one each and meet as 2 before they reach chain 0
    assert R.sum_tree(x, 1.0, np.float32) == np.float32(2.0 ** 24 + 2)
    assert R.sum_tree(x, 1.0) == 2.0 ** 24 + 3
