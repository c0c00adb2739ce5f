"""ONE attention step as include/nabu_hip.h defines it (nabu_attn_fwd / nabu_attn_bwd), restated in plain NumPy: what
tests/test_hip_attention.py holds the kernels of speller.hip to, element by element.  tests/test_attn_step_ref.py pins
it on the CPU against torch autograd in float64 and against one step of oracle.nabu_oracle.speller_fwd.

Everything is evaluated in `dtype`: float64 is the reference, float32 the evaluation whose distance from float64 is
the unit the device's error is measured in.  kind and prob_fn are the integers of nabu_attn_desc (0 vanilla,
1 location_aware, 2 windowed; 0 softmax, 1 sigmoid, 2 normalized_sigmoid); K, F are filtersize, numfilt for
location-aware attention and left_window_width, right_window_width for windowed attention."""
import numpy as np

from oracle import nabu_oracle as O

PROB_FN_NAMES = ('softmax', 'sigmoid', 'normalized_sigmoid')


def n_slices(B, Te):
    """frame slices per utterance of both passes: S = min(ceil(512 / B), ceil(Te / 16), 8)"""
    return max(1, min(-(-512 // B), -(-Te // 16), 8))


def window_bounds(align_prev, left, right):
    """first and one-past-last frame of the window [max(m - left - 1, 0), min(m + right, Te)) per utterance, m the first
    frame whose cumulated previous alignment exceeds 0.5 (Te if none does); also m and the cumulated alignment"""
    Te = align_prev.shape[1]
    cum = np.cumsum(align_prev, 1)
    over = cum > 0.5
    m = np.where(over.any(1), over.argmax(1), Te)
    return np.maximum(m - left - 1, 0), np.minimum(m + right, Te), m, cum


def slice_bounds(Te, S, n):
    """frames [lo, hi) that slice sl = 0..S-1 of an utterance of n valid frames owns"""
    per = -(-Te // S)
    return [(min(sl * per, n), min(sl * per + per, n)) for sl in range(S)]


def attn_step_fwd(kind, prob_fn, K, F, step, dec_len, enc_len, keys, values, q, v, conv_kernel, conv_proj, align_prev,
                  ctx_prev, dtype=np.float64):
    """returns align [B,Te], ctx [B,E], znorm [B] (the normaliser of normalized_sigmoid, None for the other
    probability functions) and the cache attn_step_bwd needs.  Rows with step >= dec_len[b] are finished: they return
    align_prev / ctx_prev unchanged (their znorm entry means nothing)."""
    cast = lambda a: None if a is None else np.asarray(a).astype(dtype)
    keys, values, q, v, align_prev, ctx_prev = map(cast, (keys, values, q, v, align_prev, ctx_prev))
    conv_kernel, conv_proj = cast(conv_kernel), cast(conv_proj)
    B, Te, U = keys.shape
    enc_len, dec_len = np.asarray(enc_len), np.asarray(dec_len)
    live = step < dec_len
    mask = np.arange(Te)[None, :] < enc_len[:, None]
    s = keys + q[:, None, :]
    cf = None
    if kind == 1:
        cf = O.conv1d_same(align_prev, conv_kernel)                # [B,Te,F]
        s = s + cf @ conv_proj
    th = np.tanh(s)
    score = th @ v
    pmask = mask
    if kind == 2:
        w_lo, w_hi, _, _ = window_bounds(align_prev, K, F)
        t = np.arange(Te)[None, :]
        pmask = mask & (t >= w_lo[:, None]) & (t < w_hi[:, None])
    name = PROB_FN_NAMES[prob_fn]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):     # (finished rows may have no frame to attend)
        al = O._prob_fwd(score, pmask, name)
        znorm = np.where(pmask, O.sigmoid(score), 0).sum(1) if prob_fn == 2 else None
    al = np.where(live[:, None], al, 0).astype(dtype)
    cx = np.einsum('bt,bte->be', al, values)
    align = np.where(live[:, None], al, align_prev)
    ctx = np.where(live[:, None], cx, ctx_prev)
    cache = dict(kind=kind, prob_fn=prob_fn, K=K, F=F, live=live, enc_len=enc_len, pmask=pmask, keys=keys, values=values,
                 v=v, conv_kernel=conv_kernel, conv_proj=conv_proj, align_prev=align_prev, cf=cf, th=th, score=score,
                 al=al, dtype=dtype)
    return align, ctx, znorm, cache


def attn_step_bwd(cache, dctx, dalign_in, S):
    """gradient of attn_step_fwd for d ctx [B,E] and (optionally) d align [B,Te]: returns dq [B,U], dkeys [B,Te,U] (the
    increment), dv_part [B*S,U], dconv_proj_part [B*S,F,U], dconv_kernel_part [B,K,F] (the increments; the last two None
    unless location-aware) and dalign_out [B,Te].  Row b*S + sl of a partial holds the frame sums over slice sl's frames
    [min(sl*per, n), min(sl*per + per, n)), per = ceil(Te / S), n = enc_len[b].  dalign_out is the gradient with respect
    to align_prev at all Te frames for location-aware attention and zero for the other kinds; for a finished row it is
    dalign_in (zero without one).  Finished rows have dq = 0 and add nothing anywhere."""
    dt = cache['dtype']
    kind, live, enc_len = cache['kind'], cache['live'], cache['enc_len']
    values, v, th, al = cache['values'], cache['v'], cache['th'], cache['al']
    B, Te, U = th.shape
    dctx = np.asarray(dctx).astype(dt)
    din = np.zeros((B, Te), dt) if dalign_in is None else np.asarray(dalign_in).astype(dt)
    dal = np.einsum('be,bte->bt', dctx, values) + din
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        dscore = O._prob_bwd(dal, al, cache['score'], cache['pmask'], PROB_FN_NAMES[cache['prob_fn']])
    dscore = np.where(live[:, None] & cache['pmask'], dscore, 0).astype(dt)
    ds = dscore[:, :, None] * v * (1 - th * th)                    # d (keys + q + location features) [B,Te,U]
    dkeys = ds
    dq = ds.sum(1)
    dv_part = np.zeros((B * S, U), dt)
    loc = kind == 1
    cf, cp, ck = cache['cf'], cache['conv_proj'], cache['conv_kernel']
    dcp_part = np.zeros((B * S,) + cp.shape, dt) if loc else None
    for b in range(B):
        for sl, (lo, hi) in enumerate(slice_bounds(Te, S, int(enc_len[b]))):
            dv_part[b * S + sl] = dscore[b, lo:hi] @ th[b, lo:hi]
            if loc:
                dcp_part[b * S + sl] = cf[b, lo:hi].T @ ds[b, lo:hi]
    dck_part = None
    dalign_out = np.zeros((B, Te), dt)
    if loc:
        dcf = ds @ cp.T                                            # [B,Te,F]
        dck_part = np.zeros((B,) + ck.shape, dt)
        for b in range(B):
            da, dck_part[b] = O.conv1d_same_bwd(dcf[b:b + 1], cache['align_prev'][b:b + 1], ck)
            dalign_out[b] = da[0]
    dalign_out = np.where(live[:, None], dalign_out, din)
    return dq, dkeys, dv_part, dcp_part, dck_part, dalign_out
