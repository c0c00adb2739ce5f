"""The one restatement self_attn_bf16.hip adds to tests/self_attn_ref.py: attn_bwd's formulas in float32 with P and dS
rounded to bf16 (round to nearest even) where the kernels round them.  qkv and do are taken as they come: the tests
round them before upload, so Q, K, V and dO round to themselves."""
import numpy as np

from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_ref import _heads


def attn_bwd_bf16(qkv, lse, do, lens, H):
    """dqkv [B,T,3D] in float32 from the float32 lse: P = exp(S - lse) (fp32); o = bf16(P) V and dV = bf16(P)^T dO;
    delta = rowsum(dO . o); dS = P . (dO V^T - delta) (fp32); dQ = bf16(dS) K / sqrt(dk), dK = bf16(dS)^T Q / sqrt(dk)"""
    f = np.float32
    qkv, lse, do = (a.astype(f) for a in (qkv, lse, do))
    B, T, D = do.shape
    dqkv, scale = np.zeros(qkv.shape, f), f(1 / np.sqrt(D // H))
    for b, L in enumerate(np.clip(lens, 0, T)):
        if L == 0:
            continue
        q, k, v = _heads(qkv, b, L, H)
        doh = do[b, :L].reshape(L, H, D // H).transpose(1, 0, 2)
        p = np.exp(np.einsum('hid,hjd->hij', q, k) * scale - lse[b, :, :L, None])
        p16 = bf16_rne(p)[1]
        delta = (doh * np.einsum('hij,hjd->hid', p16, v)).sum(2, keepdims=True)
        ds16 = bf16_rne(p * (np.einsum('hid,hjd->hij', doh, v) - delta))[1]
        for i, g in enumerate((np.einsum('hij,hjd->hid', ds16, k) * scale, np.einsum('hij,hid->hjd', ds16, q) * scale,
                               np.einsum('hij,hid->hjd', p16, doh))):
            dqkv[b, :L, i * D:(i + 1) * D] = g.transpose(1, 0, 2).reshape(L, D)
    return dqkv
