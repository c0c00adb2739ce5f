"""Plain restatement of conv_module.hip and of layer.conformer_block as torch CPU compositions at a given dtype (float64:
the reference; float32: the reference's own rounding floor).  The operation runs for ONE utterance at its own length;
a batch is the utterances one by one, zero rows past each length.  Every gradient is torch.autograd.grad's."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import self_attn_ref as R

EPS = 1e-5
CORE = ('y', 'du', 'dw', 'dbw', 'dgamma', 'dbeta')


def core(u, w, bw, gamma, beta):
    """u [L,2D] -> y [L,D]: GLU, depthwise "same" convolution along time, layer norm per frame, Swish"""
    K, D = w.shape
    g = u[:, :D] * torch.sigmoid(u[:, D:])
    z = F.conv1d(g.t()[None], w.t()[:, None, :], bw, padding=(K - 1) // 2, groups=D)[0].t()
    n = F.layer_norm(z, (D,), gamma, beta, EPS)
    return n * torch.sigmoid(n)


def batch_core(u, lens, w, bw, gamma, beta):
    """u [B,T,2D] -> y [B,T,D], rows >= len zero"""
    T, D = u.shape[1], w.shape[1]
    return torch.stack([F.pad(core(u[b, :L], w, bw, gamma, beta), (0, 0, 0, T - L)) if L else u.new_zeros((T, D))
                        for b, L in enumerate(int(v) for v in np.clip(lens, 0, T))])


def conv_module(u, lens, w, bw, gamma, beta, dy, dtype=torch.float64):
    """{name: array} for the names of CORE, from numpy operands"""
    u, w, bw, gamma, beta = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (u, w, bw, gamma, beta))
    y = batch_core(u, lens, w, bw, gamma, beta)
    grads = torch.autograd.grad(y, (u, w, bw, gamma, beta), torch.tensor(dy, dtype=dtype))
    return {n: t.detach().numpy() for n, t in zip(CORE, (y,) + grads)}


def swish(x, dy, dtype=torch.float64):
    """(x sigmoid(x), its gradient at x times dy)"""
    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    y = x * torch.sigmoid(x)
    return y.detach().numpy(), torch.autograd.grad(y, x, torch.tensor(dy, dtype=dtype))[0].numpy()


class _Attention(torch.autograd.Function):
    """tests/self_attn_ref.py's attention as a node of the graph"""
    @staticmethod
    def forward(ctx, qkv, lens, H):
        o, lse = R.attn_fwd(qkv.numpy(), lens, H)
        ctx.kept = (qkv.numpy(), o, lse, lens, H)
        return torch.from_numpy(o)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, lens, H = ctx.kept
        return torch.from_numpy(R.attn_bwd(qkv, o, lse, do.numpy(), lens, H)), None, None


NAMES = ['%s/%s' % (n, p) for n in ('ln_ff1', 'ln_att', 'ln_conv', 'ln_ff2', 'ln_out', 'conv/norm') for p in ('gamma', 'beta')] + \
    ['%s/%s' % (n, p) for n in ('ffn1/fc1', 'ffn1/fc2', 'attention/qkv', 'attention/out', 'conv/pw1', 'conv/pw2', 'ffn2/fc1',
                                'ffn2/fc2') for p in ('weights', 'biases')] + ['conv/dw/kernel', 'conv/dw/bias']


def block(h, lens, P, H, dout):
    """layer.conformer_block without dropout in float64; P: {name: array} by NAMES.  (out, dh, {name: gradient})"""
    h = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    P = {n: torch.tensor(P[n], dtype=torch.float64, requires_grad=True) for n in NAMES}
    D = h.shape[-1]

    def ln(x, n):
        return F.layer_norm(x, (D,), P[n + '/gamma'], P[n + '/beta'], EPS)

    def lin(x, n):
        return x @ P[n + '/weights'] + P[n + '/biases']

    def ffn(x, n, norm):
        y = lin(ln(x, norm), n + '/fc1')
        return x + 0.5 * lin(y * torch.sigmoid(y), n + '/fc2')
    x = ffn(h, 'ffn1', 'ln_ff1')
    x = x + lin(_Attention.apply(lin(ln(x, 'ln_att'), 'attention/qkv'), lens, H), 'attention/out')
    v = batch_core(lin(ln(x, 'ln_conv'), 'conv/pw1'), lens, P['conv/dw/kernel'], P['conv/dw/bias'], P['conv/norm/gamma'],
                   P['conv/norm/beta'])
    out = ln(ffn(x + lin(v, 'conv/pw2'), 'ffn2', 'ln_ff2'), 'ln_out')
    grads = torch.autograd.grad(out, [h] + [P[n] for n in NAMES], torch.tensor(dout, dtype=torch.float64))
    return out.detach().numpy(), grads[0].numpy(), {n: g.numpy() for n, g in zip(NAMES, grads[1:])}
