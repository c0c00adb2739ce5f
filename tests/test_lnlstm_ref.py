"""CPU tests that pin the yardstick of the layer-normalised BLSTM kernels: the NumPy restatement tests/lnlstm_ref.py
(forward + hand-written backward) against float64 torch autograd of an INDEPENDENT forward written with
torch.nn.functional.layer_norm(eps=1e-12)."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from tests import lnlstm_ref as R


def torch_forward(x, lens, p):
    """the layer in torch float64, one utterance at a time (no masking logic shared with the restatement)"""
    B, T, D = x.shape
    H = p['fw_kernel'].shape[1] // 4
    F = torch.nn.functional
    rows = []
    for b in range(B):
        n = int(lens[b])
        halves = []
        for d, order in (('fw', range(n)), ('bw', range(n - 1, -1, -1))):
            W, gam, bet = p[d + '_kernel'], p[d + '_gamma'], p[d + '_beta']
            h = torch.zeros(H, dtype=torch.float64)
            c = torch.zeros(H, dtype=torch.float64)
            outs = [None] * T
            for t in order:
                z = torch.cat([x[b, t], h]) @ W
                y = [F.layer_norm(z[k * H:(k + 1) * H], (H,), gam[k], bet[k], eps=1e-12) for k in range(4)]
                c = c * torch.sigmoid(y[2] + 1.0) + torch.sigmoid(y[0]) * torch.tanh(y[1])
                c = F.layer_norm(c, (H,), gam[4], bet[4], eps=1e-12)
                h = torch.tanh(c) * torch.sigmoid(y[3])
                outs[t] = h
            zero = torch.zeros(H, dtype=torch.float64)
            halves.append(torch.stack([o if o is not None else zero for o in outs]))
        rows.append(torch.cat(halves, 1))
    return torch.stack(rows)


@pytest.mark.parametrize('B,T,D,H,lens', [(3, 6, 5, 8, [6, 1, 4]), (2, 9, 7, 12, [5, 9])])
def test_restatement_gradients_equal_torch_autograd(B, T, D, H, lens):
    rng = np.random.default_rng(7)
    p = R.init_params(rng, D, H, perturb=0.3)
    x = rng.standard_normal((B, T, D))
    dout = rng.standard_normal((B, T, 2 * H))
    out, cache = R.blstm_fwd(x, lens, p)
    dx, grads = R.blstm_bwd(dout, cache)
    tp = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tout = torch_forward(tx, lens, tp)
    (tout * torch.tensor(dout)).sum().backward()

    def rel(a, b):
        return np.abs(a - b).max() / np.abs(b).max()
    assert rel(out, tout.detach().numpy()) <= 1e-9
    assert rel(dx, tx.grad.numpy()) <= 1e-9
    for k in grads:
        assert rel(grads[k], tp[k].grad.numpy()) <= 1e-9, k
    for b, n in enumerate(lens):
        assert not out[b, n:].any() and not dx[b, n:].any()


def test_unit_gamma_zero_beta_is_not_the_plain_layer():
    """a no-op norm would pass every parity test against itself: gamma = 1, beta = 0 must differ from the oracle's
    layer without layer norm on the same kernels"""
    rng = np.random.default_rng(3)
    B, T, D, H = 3, 7, 8, 16
    p = R.init_params(rng, D, H)
    x = rng.standard_normal((B, T, D))
    lens = [7, 3, 5]
    out, _ = R.blstm_fwd(x, lens, p)
    plain, _ = O.blstm_fwd(x, np.asarray(lens), dict(fw_kernel=p['fw_kernel'], fw_bias=np.zeros(4 * H),
                                                      bw_kernel=p['bw_kernel'], bw_bias=np.zeros(4 * H)))
    assert out.shape == plain.shape
    assert np.abs(out - plain).max() > 0.05


def test_variable_names():
    names = R.variable_shapes(40, 64)
    assert len(names) == 2 * 11
    cell = 'bidirectional_rnn/fw/layer_norm_basic_lstm_cell/'
    assert names[0] == (cell + 'kernel', (104, 256))
    assert [n for n, _ in names[1:11]] == [cell + s + '/' + w for s in ('input', 'transform', 'forget', 'output', 'state')
                                           for w in ('gamma', 'beta')]
    assert all(s == (64,) for _, s in names[1:11])
    assert names[11][0] == 'bidirectional_rnn/bw/layer_norm_basic_lstm_cell/kernel'
    assert not any(n.endswith('bias') for n, _ in names)


def test_float32_evaluation_follows_the_dtype():
    """the yardstick of the GPU test is this restatement evaluated in float32: nothing in it may promote to float64"""
    rng = np.random.default_rng(5)
    p = R.cast(R.init_params(rng, 6, 8, perturb=0.2), np.float32)
    x = rng.standard_normal((2, 5, 6)).astype(np.float32)
    out, cache = R.blstm_fwd(x, [5, 2], p)
    dx, grads = R.blstm_bwd(rng.standard_normal((2, 5, 16)).astype(np.float32), cache)
    assert out.dtype == dx.dtype == np.float32
    assert all(g.dtype == np.float32 for g in grads.values())
    assert R.min_variance(cache) > 1e-6
