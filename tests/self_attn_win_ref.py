"""Restatement of the chunk-limited attention (nabu_self_attn[_bf16]_win_*): tests/self_attn_ref.py's formulas on the full
score matrix under the mask lo(i) <= j < hi(i), optionally with the dropout mask d of tests/self_attn_drop_ref.py on top.
float64 is the reference, float32 its rounding floor; bf16=True rounds (d . P) and dS where the bf16 kernels round them."""
import numpy as np

from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_ref import _heads


def visible(L, C, Lc):
    """[L, L] bool: query i sees key j iff lo(i) <= j < hi(i); hi = min(L, (i // C + 1) C), lo = 0 if Lc < 0 else
    max(0, (i // C - Lc) C)"""
    c, j = np.arange(L)[:, None] // C, np.arange(L)[None, :]
    return (j < np.minimum(L, (c + 1) * C)) & (j >= (0 if Lc < 0 else np.maximum(0, (c - Lc) * C)))


def attn_fwd_win(qkv, lens, H, window, d=None, dtype=np.float64, bf16=False):
    """(o [B,T,D], lse [B,H,T]): softmax and lse over the visible keys, undropped; o = (d . P) V (bf16: the unnormalised
    d . p is rounded)"""
    qkv = qkv.astype(dtype)
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    o, lse = np.zeros((B, T, D), dtype), np.zeros((B, H, T), dtype)
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L:
            q, k, v = _heads(qkv, b, L, H)
            s = np.where(visible(L, *window), np.einsum('hid,hjd->hij', q, k) * dtype(1 / np.sqrt(D // H)), dtype(-np.inf))
            m = s.max(2, keepdims=True)
            p, dd = np.exp(s - m), dtype(1) if d is None else d[b, :, :L, :L].astype(dtype)
            l = p.sum(2, keepdims=True)
            num = np.einsum('hij,hjd->hid', bf16_rne(p * dd)[1] if bf16 else p / l * dd, v)
            o[b, :L] = (num / l if bf16 else num).transpose(1, 0, 2).reshape(L, D)
            lse[b, :, :L] = (m + np.log(l))[:, :, 0]
    return o, lse


def attn_bwd_win(qkv, o, lse, do, lens, H, window, d=None, dtype=np.float64, bf16=False):
    """dqkv [B,T,3D]: P = exp(s - lse) on the visible keys and 0 elsewhere; delta = rowsum(dO . o), dP = d . (dO V^T),
    dS = P . (dP - delta), dQ = dS K / sqrt(dk), dK = dS^T Q / sqrt(dk), dV = (d . P)^T dO"""
    qkv, o, lse, do = (a.astype(dtype) for a in (qkv, o, lse, do))
    B, T, D = o.shape
    dqkv, scale = np.zeros(qkv.shape, dtype), dtype(1 / np.sqrt(D // H))
    rnd = (lambda x: bf16_rne(x)[1]) if bf16 else (lambda x: x)
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L:
            q, k, v = _heads(qkv, b, L, H)
            oh, doh = (a[b, :L].reshape(L, H, D // H).transpose(1, 0, 2) for a in (o, do))
            dd = dtype(1) if d is None else d[b, :, :L, :L].astype(dtype)
            p = np.where(visible(L, *window), np.exp(np.einsum('hid,hjd->hij', q, k) * scale - lse[b, :, :L, None]), dtype(0))
            ds = rnd(p * (np.einsum('hid,hjd->hij', doh, v) * dd - (doh * oh).sum(2, keepdims=True)))
            for i, g in enumerate((np.einsum('hij,hjd->hid', ds, k) * scale, np.einsum('hij,hid->hjd', ds, q) * scale,
                                   np.einsum('hij,hid->hjd', rnd(p * dd), doh))):
                dqkv[b, :L, i * D:(i + 1) * D] = g.transpose(1, 0, 2).reshape(L, D)
    return dqkv
