"""Restatement of the attention with dropout on its probabilities (nabu_self_attn[_bf16]_drop_*, include/nabu_hip.h):
tests/self_attn_ref.py's formulas on the full score matrix with the mask d in {0, fl(1 / keep)} from the host Philox.
float64 is the reference, float32 its rounding floor; bf16=True rounds (d . P) and dS where the bf16 kernels round them."""
import numpy as np

from oracle.philox import philox4x32_10, u01
from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_ref import _heads


def keep_scale(B, H, T, keep, seed, offset):
    """d [B,H,T,T] float32: element (b,h,q,k) is word k & 3 of the block with counter (g_lo, g_hi, offset_lo, offset_hi),
    key (seed_lo, seed_hi), g = ((b H + h) << 38) | (q << 18) | (k >> 2); fl(1 / keep) where u01(word) < keep, else 0"""
    u, lo = np.uint64, 0xFFFFFFFF
    bh, q, kg = np.meshgrid(np.arange(B * H, dtype=u), np.arange(T, dtype=u), np.arange((T + 3) // 4, dtype=u), indexing='ij')
    g = (bh << u(38)) | (q << u(18)) | kg
    ctr = np.stack([g & u(lo), g >> u(32), np.full_like(g, offset & lo), np.full_like(g, offset >> 32)], -1).astype(np.uint32)
    words = philox4x32_10(ctr, np.array([seed & lo, seed >> 32], np.uint32)).reshape(B, H, T, -1)[..., :T]
    return np.where(u01(words) < np.float64(np.float32(keep)), np.float32(1) / np.float32(keep), np.float32(0)).astype(np.float32)


def attn_fwd_drop(qkv, lens, H, d, dtype=np.float64, bf16=False):
    """(o [B,T,D], lse [B,H,T]): P = softmax, undropped like lse; o = (d . P) V (bf16: the unnormalised d . p is rounded)"""
    qkv = qkv.astype(dtype)
    B, T, D = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    o, lse = np.zeros((B, T, D), dtype), np.zeros((B, H, T), dtype)
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L:
            q, k, v = _heads(qkv, b, L, H)
            s = np.einsum('hid,hjd->hij', q, k) * dtype(1 / np.sqrt(D // H))
            m = s.max(2, keepdims=True)
            p, dd = np.exp(s - m), d[b, :, :L, :L].astype(dtype)
            l = p.sum(2, keepdims=True)
            num = np.einsum('hij,hjd->hid', bf16_rne(p * dd)[1] if bf16 else p / l * dd, v)
            o[b, :L] = (num / l if bf16 else num).transpose(1, 0, 2).reshape(L, D)
            lse[b, :, :L] = (m + np.log(l))[:, :, 0]
    return o, lse


def attn_bwd_drop(qkv, o, lse, do, lens, H, d, dtype=np.float64, bf16=False):
    """dqkv [B,T,3D]: delta = rowsum(dO . o), dP = d . (dO V^T), dS = P . (dP - delta), dQ = dS K / sqrt(dk),
    dK = dS^T Q / sqrt(dk), dV = (d . P)^T dO"""
    qkv, o, lse, do = (a.astype(dtype) for a in (qkv, o, lse, do))
    B, T, D = o.shape
    dqkv, scale = np.zeros(qkv.shape, dtype), dtype(1 / np.sqrt(D // H))
    rnd = (lambda x: bf16_rne(x)[1]) if bf16 else (lambda x: x)
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L:
            q, k, v = _heads(qkv, b, L, H)
            oh, doh = (a[b, :L].reshape(L, H, D // H).transpose(1, 0, 2) for a in (o, do))
            dd = d[b, :, :L, :L].astype(dtype)
            p = np.exp(np.einsum('hid,hjd->hij', q, k) * scale - lse[b, :, :L, None])
            ds = rnd(p * (np.einsum('hid,hjd->hij', doh, v) * dd - (doh * oh).sum(2, keepdims=True)))
            for i, g in enumerate((np.einsum('hij,hjd->hid', ds, k) * scale, np.einsum('hij,hid->hjd', ds, q) * scale,
                                   np.einsum('hij,hid->hjd', rnd(p * dd), doh))):
                dqkv[b, :L, i * D:(i + 1) * D] = g.transpose(1, 0, 2).reshape(L, D)
    return dqkv
