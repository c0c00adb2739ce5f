"""Textbook restatement of self_attn.hip and of layer.self_attention_block: the full score matrix with lengths, in float64
(or, with dtype=np.float32, the same formulas at the kernels' precision: the reference's own rounding floor).
qkv [B,T,3D]: Q, K, V are the three D-wide column blocks, head h is columns h dk .. (h+1) dk of each.  Keys >= len do
not exist; rows >= len of every result are zero."""
import numpy as np

from tests.conv_ref import gamma          # noqa: F401  (n u / (1 - n u))

EPS = 1e-5


def _heads(qkv, b, L, H):
    D = qkv.shape[2] // 3
    return [qkv[b, :L, i * D:(i + 1) * D].reshape(L, H, D // H).transpose(1, 0, 2) for i in range(3)]     # [H,L,dk] each


def attn_fwd(qkv, lens, H, dtype=np.float64, bound=False):
    """(o [B,T,D], lse [B,H,T]); bound=True: also E[b,h,t] = max_j |q|.|k_j| / sqrt(dk) and A [B,T,D] = sum_j p_j |v_j|"""
    qkv = qkv.astype(dtype)
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    o, lse = np.zeros((B, T, D), dtype), np.zeros((B, H, T), dtype)
    E, A = np.zeros((B, H, T)), np.zeros((B, T, D))
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L == 0:
            continue
        q, k, v = _heads(qkv, b, L, H)
        s = np.einsum('hid,hjd->hij', q, k) * dtype(1 / np.sqrt(D // H))
        m = s.max(2, keepdims=True)
        p = np.exp(s - m)
        l = p.sum(2, keepdims=True)
        p = p / l
        o[b, :L] = np.einsum('hij,hjd->ihd', p, v).reshape(L, D)
        lse[b, :, :L] = (m + np.log(l))[:, :, 0]
        if bound:
            E[b, :, :L] = (np.einsum('hid,hjd->hij', np.abs(q), np.abs(k)) / np.sqrt(D // H)).max(2)
            A[b, :L] = np.einsum('hij,hjd->ihd', p, np.abs(v)).reshape(L, D)
    return (o, lse, E, A) if bound else (o, lse)


def attn_bwd(qkv, o, lse, do, lens, H, dtype=np.float64):
    """dqkv [B,T,3D]: delta = rowsum(do . o), dV = P^T dO, dS = P . (dO V^T - delta), dQ = dS K / sqrt(dk), dK = dS^T Q / sqrt(dk)"""
    qkv, o, lse, do = (a.astype(dtype) for a in (qkv, o, lse, do))
    B, T, D = o.shape
    dqkv = np.zeros(qkv.shape, dtype)
    scale = dtype(1 / np.sqrt(D // H))
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L == 0:
            continue
        q, k, v = _heads(qkv, b, L, H)
        oh, doh = (a[b, :L].reshape(L, H, D // H).transpose(1, 0, 2) for a in (o, do))
        p = np.exp(np.einsum('hid,hjd->hij', q, k) * scale - lse[b, :, :L, None])
        ds = p * (np.einsum('hid,hjd->hij', doh, v) - (doh * oh).sum(2, keepdims=True))
        for i, g in enumerate((np.einsum('hij,hjd->hid', ds, k) * scale, np.einsum('hij,hid->hjd', ds, q) * scale,
                               np.einsum('hij,hid->hjd', p, doh))):
            dqkv[b, :L, i * D:(i + 1) * D] = g.transpose(1, 0, 2).reshape(L, D)
    return dqkv


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdims=True)
    rstd = 1 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + EPS)
    return (x - mu) * rstd * g + b, ((x - mu) * rstd, rstd)


def layer_norm_bwd(dy, g, cache):
    xhat, rstd = cache
    dg = dy * g
    dx = rstd * (dg - dg.mean(-1, keepdims=True) - xhat * (dg * xhat).mean(-1, keepdims=True))
    return dx, (dy * xhat).reshape(-1, dy.shape[-1]).sum(0), dy.reshape(-1, dy.shape[-1]).sum(0)


NAMES = ['ln1/gamma', 'ln1/beta', 'ln2/gamma', 'ln2/beta'] + \
    ['%s/%s' % (n, w) for n in ('attention/qkv', 'attention/out', 'ffn/fc1', 'ffn/fc2') for w in ('weights', 'biases')]


def block_fwd(h, lens, P, H):
    """the pre-norm block of layer.self_attention_block without dropout; P: {name: array} by NAMES.  (out, cache)"""
    a, c1 = layer_norm(h, P['ln1/gamma'], P['ln1/beta'])
    qkv = a @ P['attention/qkv/weights'] + P['attention/qkv/biases']
    c, lse = attn_fwd(qkv, lens, H)
    h1 = h + c @ P['attention/out/weights'] + P['attention/out/biases']
    f, c2 = layer_norm(h1, P['ln2/gamma'], P['ln2/beta'])
    r = np.maximum(f @ P['ffn/fc1/weights'] + P['ffn/fc1/biases'], 0)
    return h1 + r @ P['ffn/fc2/weights'] + P['ffn/fc2/biases'], (h, lens, P, H, a, c1, qkv, c, lse, f, c2, r)


def block_bwd(dout, cache):
    """({name: gradient}, dh)"""
    h, lens, P, H, a, c1, qkv, c, lse, f, c2, r = cache
    G = {}

    def linear(x, dy, name):
        G[name + '/weights'] = x.reshape(-1, x.shape[-1]).T @ dy.reshape(-1, dy.shape[-1])
        G[name + '/biases'] = dy.reshape(-1, dy.shape[-1]).sum(0)
        return dy @ P[name + '/weights'].T
    du = linear(r, dout, 'ffn/fc2') * (r > 0)
    dh1, G['ln2/gamma'], G['ln2/beta'] = layer_norm_bwd(linear(f, du, 'ffn/fc1'), P['ln2/gamma'], c2)
    dh1 = dh1 + dout
    dqkv = attn_bwd(qkv, c, lse, linear(c, dh1, 'attention/out'), lens, H)
    dh, G['ln1/gamma'], G['ln1/beta'] = layer_norm_bwd(linear(a, dqkv, 'attention/qkv'), P['ln1/gamma'], c1)
    return G, dh + dh1
