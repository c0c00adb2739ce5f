"""CPU: tests/attn_step_ref.py (the restatement of ONE attention step that tests/test_hip_attention.py holds the kernels
to) against torch autograd in float64 on the written-out formulas, against one step of the oracle's whole decoder, and
the ownership rule of its per-slice partial sums."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from tests import attn_step_ref as R

KINDS = ('vanilla', 'location_aware', 'windowed')


def _case(kind, prob_fn, B=4, Te=11, U=6, E=5, K=5, F=3, seed=0, enc_len=None, dec_len=None):
    """operands of one step; windowed: K, F = left, right.  Row 1 is finished at step 2."""
    rng = np.random.default_rng(seed + 10 * kind + prob_fn)
    n = lambda *s: rng.standard_normal(s)
    enc_len = np.array([Te, 7, 4, 9][:B], np.int32) if enc_len is None else enc_len
    dec_len = np.array([5, 2, 3, 4][:B], np.int32) if dec_len is None else dec_len
    mask = np.arange(Te)[None, :] < enc_len[:, None]
    sc = 1.5 * n(B, Te)
    if prob_fn == 1:
        ap = np.where(mask, O.sigmoid(sc - 2.0), 0)
    else:
        ap = O._prob_fwd(sc, mask, 'softmax')
    k = dict(kind=kind, prob_fn=prob_fn, K=K, F=F, step=2, dec_len=dec_len, enc_len=enc_len,
             keys=0.7 * n(B, Te, U), values=n(B, Te, E) * mask[:, :, None], q=0.7 * n(B, U), v=n(U),
             conv_kernel=n(K, F) if kind == 1 else None, conv_proj=0.6 * n(F, U) if kind == 1 else None,
             align_prev=ap, ctx_prev=n(B, E))
    k['dctx'], k['dalign_in'] = n(B, E), n(B, Te)
    return k


def _fwd(k, dtype=np.float64):
    return R.attn_step_fwd(k['kind'], k['prob_fn'], k['K'], k['F'], k['step'], k['dec_len'], k['enc_len'], k['keys'],
                           k['values'], k['q'], k['v'], k['conv_kernel'], k['conv_proj'], k['align_prev'],
                           k['ctx_prev'], dtype=dtype)


def _torch_step(k, b, with_dalign):
    """utterance b of the step written out in torch (the formulas of tests/torch_ref.py speller()): alignments, context
    and the gradients of sum(ctx dctx) + sum(align dalign_in) by autograd"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    kind, pf = k['kind'], k['prob_fn']
    Te = k['keys'].shape[1]
    n = int(k['enc_len'][b])
    leaf = lambda a: t(a).requires_grad_(True)
    keys, q, v, al_prev = leaf(k['keys'][b]), leaf(k['q'][b]), leaf(k['v']), leaf(k['align_prev'][b])
    values = t(k['values'][b])
    ck = cp = None
    s = keys + q[None, :]
    if kind == 1:
        ck, cp = leaf(k['conv_kernel']), leaf(k['conv_proj'])
        Kw = ck.shape[0]
        pb = (Kw - 1) // 2
        padded = torch.cat([al_prev.new_zeros(pb), al_prev, al_prev.new_zeros(Kw - 1 - pb)])
        cf = torch.nn.functional.conv1d(padded[None, None, :], ck.t()[:, None, :])[0].t()       # [Te,F]
        s = s + cf @ cp
    score = torch.tanh(s) @ v
    valid = torch.arange(Te) < n
    if kind == 2:
        over = (torch.cumsum(al_prev.detach(), 0) > 0.5).nonzero()
        m = int(over[0]) if len(over) else Te
        idx = torch.arange(Te)
        valid = valid & (idx >= m - k['K'] - 1) & (idx < m + k['F'])
    if pf == 0:
        al = torch.softmax(torch.where(valid, score, torch.full_like(score, -float('inf'))), 0)
        z = None
    else:
        sg = torch.where(valid, torch.sigmoid(score), torch.zeros_like(score))
        z = sg.sum()
        al = sg if pf == 1 else sg / z
    ctx = al @ values
    loss = (ctx * t(k['dctx'][b])).sum()
    if with_dalign:
        loss = loss + (al * t(k['dalign_in'][b])).sum()
    loss.backward()
    g = lambda x: None if x is None else (x.grad.numpy() if x.grad is not None else np.zeros(tuple(x.shape)))
    return dict(align=al.detach().numpy(), ctx=ctx.detach().numpy(), znorm=None if z is None else float(z.detach()),
                dkeys=g(keys), dq=g(q), dv=g(v), dalign_prev=g(al_prev), dck=g(ck), dcp=g(cp))


def _check_against_autograd(k, with_dalign, S=1):
    B, Te, U = k['keys'].shape
    align, ctx, znorm, cache = _fwd(k)
    din = k['dalign_in'] if with_dalign else None
    dq, dkeys, dv_part, dcp_part, dck_part, dalign_out = R.attn_step_bwd(cache, k['dctx'], din, S)
    close = lambda a, b_: np.testing.assert_allclose(a, b_, rtol=1e-11, atol=1e-13)
    assert dv_part.shape == (B * S, U)
    some_live = False
    for b in range(B):
        if k['step'] >= k['dec_len'][b]:                       # finished: frozen state, no gradient of its own
            np.testing.assert_array_equal(align[b], k['align_prev'][b])
            np.testing.assert_array_equal(ctx[b], k['ctx_prev'][b])
            assert not dq[b].any() and not dkeys[b].any() and not dv_part[b * S:(b + 1) * S].any()
            if k['kind'] == 1:
                assert not dcp_part[b * S:(b + 1) * S].any() and not dck_part[b].any()
            np.testing.assert_array_equal(dalign_out[b], din[b] if with_dalign else np.zeros(Te))
            continue
        some_live = True
        r = _torch_step(k, b, with_dalign)
        close(align[b], r['align'])
        close(ctx[b], r['ctx'])
        if k['prob_fn'] == 2:
            close(znorm[b], r['znorm'])
        else:
            assert znorm is None
        close(dq[b], r['dq'])
        close(dkeys[b], r['dkeys'])
        close(dv_part[b * S:(b + 1) * S].sum(0), r['dv'])
        if k['kind'] == 1:
            close(dcp_part[b * S:(b + 1) * S].sum(0), r['dcp'])
            close(dck_part[b], r['dck'])
            close(dalign_out[b], r['dalign_prev'])
        else:
            assert dcp_part is None and dck_part is None and not dalign_out[b].any()
        n = int(k['enc_len'][b])
        assert not align[b, n:].any() and not dkeys[b, n:].any()
    assert some_live


@pytest.mark.parametrize('with_dalign', [False, True])
@pytest.mark.parametrize('prob_fn', [0, 1, 2])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_step_restatement_equals_autograd(kind, prob_fn, with_dalign):
    K, F = (1, 2) if kind == 2 else (5, 3)
    k = _case(kind, prob_fn, K=K, F=F)
    assert (k['step'] >= k['dec_len']).tolist() == [False, True, False, False]      # a finished row among live ones
    _check_against_autograd(k, with_dalign, S=2)


@pytest.mark.parametrize('K,F', [(4, 2), (6, 1), (23, 3), (12, 2)])
def test_location_features_with_an_even_filter_width_and_a_filter_wider_than_the_signal(K, F):
    k = _case(1, 0, K=K, F=F, seed=3)
    assert K % 2 == 0 or K > k['keys'].shape[1]
    _check_against_autograd(k, True, S=1)


@pytest.mark.parametrize('left,right,pf', [(0, 1, 0), (11, 3, 2), (2, 16, 0), (3, 2, 1)])
def test_window_is_the_interval_around_the_first_frame_past_one_half(left, right, pf):
    """also right > Te, which oracle.attention_window cannot take, and left >= Te; where attention_window applies the two
    agree frame for frame; an alignment that never reaches one half puts m at Te"""
    k = _case(2, pf, K=left, F=right, seed=5)
    Te = k['keys'].shape[1]
    if pf == 1:
        k['align_prev'][0] = 0.02                   # cumulates to 0.22: m = Te, the window is the last left + 1 frames
    lo, hi, m, _ = R.window_bounds(k['align_prev'], left, right)
    if pf == 1:
        assert m[0] == Te and lo[0] == Te - left - 1 and hi[0] == Te
    if right <= Te:
        t = np.arange(Te)[None, :]
        np.testing.assert_array_equal((t >= lo[:, None]) & (t < hi[:, None]), O.attention_window(k['align_prev'], left, right))
    _check_against_autograd(k, False, S=1)


@pytest.mark.parametrize('attention,window', [('vanilla', None), ('location_aware', None), ('windowed', (1, 2))])
def test_one_step_of_the_oracle_decoder_is_this_step(attention, window):
    rng = np.random.default_rng(8)
    B, Te, E, U, C, K, F = 3, 9, 5, 6, 7, 4, 2
    n = lambda *s: rng.standard_normal(s)
    enc_len, tlen = np.array([9, 5, 7], np.int32), np.array([4, 2, 3], np.int32)
    p = dict(memory_kernel=n(E, U), query_kernel=n(U, U), attention_v=n(U), out_kernel=n(U + E, C), out_bias=n(C),
             lstm=[dict(kernel=0.5 * n(C + E + U, 4 * U), bias=n(4 * U))])
    if attention == 'location_aware':
        p.update(conv_kernel=n(K, F), conv_proj=n(F, U))
    tg = rng.integers(0, C - 1, (B, 5))
    _, _, cache = O.speller_fwd(n(B, Te, E), enc_len, tg, tlen, p, attention, 'normalized_sigmoid', window=window)
    kind = KINDS.index(attention)
    kf = window if window else (K, F)
    for step in (0, 2, 3):
        st = cache['steps'][step]
        align, ctx, znorm, _ = R.attn_step_fwd(kind, 2, kf[0], kf[1], step, tlen, enc_len, cache['keys'], cache['values'],
                                               st['query'] @ p['query_kernel'], p['attention_v'], p.get('conv_kernel'),
                                               p.get('conv_proj'), st['align_prev'], st['ctx_prev'])
        act = st['act']
        assert act.any() and (step == 0 or not act.all())
        np.testing.assert_allclose(align, np.where(act, st['al'], st['align_prev']), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(ctx, np.where(act, st['cx'], st['ctx_prev']), rtol=1e-13, atol=1e-15)
        sg = np.where(st['pmask'], O.sigmoid(st['score']), 0).sum(1)
        np.testing.assert_allclose(znorm[act[:, 0]], sg[act[:, 0]], rtol=1e-13)


@pytest.mark.parametrize('S', [1, 2, 5, 8])
def test_slice_partials_sum_to_the_unsliced_gradient_and_respect_ownership(S):
    Te = 37
    enc_len = np.array([37, 8, 1, 20], np.int32)
    k = _case(1, 2, Te=Te, enc_len=enc_len, dec_len=np.array([5, 3, 4, 1], np.int32), seed=9)
    _, _, _, cache = _fwd(k)
    one = R.attn_step_bwd(cache, k['dctx'], k['dalign_in'], 1)
    got = R.attn_step_bwd(cache, k['dctx'], k['dalign_in'], S)
    B, U = 4, k['keys'].shape[2]
    for i in (0, 1, 4, 5):                                      # what no slicing touches
        np.testing.assert_array_equal(got[i], one[i])
    np.testing.assert_allclose(got[2].reshape(B, S, U).sum(1), one[2], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got[3].reshape(B, S, k['F'], U).sum(1), one[3], rtol=1e-12, atol=1e-14)
    per = -(-Te // S)
    for b in range(B):
        bounds = R.slice_bounds(Te, S, int(enc_len[b]))
        assert bounds[0][0] == 0 and bounds[-1][1] == enc_len[b] and all(a[1] == b_[0] for a, b_ in zip(bounds, bounds[1:]))
        for sl, (lo, hi) in enumerate(bounds):
            assert hi - lo <= per
            if hi == lo or k['step'] >= k['dec_len'][b]:       # a slice without a frame, a finished row: nothing
                assert not got[2][b * S + sl].any() and not got[3][b * S + sl].any()
            elif enc_len[b] > 1:                                # (one frame alone: its normalised alignment is the constant 1)
                assert got[2][b * S + sl].any()


def test_float32_evaluation_stays_float32_and_close():
    for kind in (0, 1, 2):
        for pf in (0, 1, 2):
            k = _case(kind, pf, K=1 if kind == 2 else 5, F=2 if kind == 2 else 3)
            k = {n_: (v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v)
                 for n_, v in k.items()}
            a64, c64, z64, cache64 = _fwd(k)
            a32, c32, z32, cache32 = _fwd(k, np.float32)
            g64 = R.attn_step_bwd(cache64, k['dctx'], k['dalign_in'], 2)
            g32 = R.attn_step_bwd(cache32, k['dctx'], k['dalign_in'], 2)
            for x32, x64 in [(a32, a64), (c32, c64), (z32, z64)] + list(zip(g32, g64)):
                if x64 is None:
                    assert x32 is None
                    continue
                assert x32.dtype == np.float32 and x64.dtype == np.float64
                assert np.abs(x32 - x64).max() <= 1e-5 * max(1.0, np.abs(x64).max())


def test_slice_count_formula():
    assert [R.n_slices(*s) for s in [(3, 13), (512, 40), (3, 17), (5, 70), (2, 130), (64, 200), (600, 400)]] == \
        [1, 1, 2, 5, 8, 8, 1]
