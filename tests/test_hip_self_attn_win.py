"""GPU: the chunk window inside the self-attention kernels (nabu_self_attn[_bf16]_win_*) against tests/self_attn_win_ref.py"""
import numpy as np
import pytest
import torch

import tests.test_hip_self_attn as plain_tests
from nabu_amd import _hip, ops as hip, recipes
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import self_attn_ref as R
from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_drop_ref import keep_scale
from tests.self_attn_win_ref import attn_bwd_win, attn_fwd_win
from tests.test_hip_self_attn import SENTINEL, clean, dev, guarded

pytestmark = pytest.mark.gpu
FACTOR = {'f32': 8.0, 'bf16': 4.0}      # the factors of tests/test_hip_self_attn_drop.py (DESIGN.md sections 15, 17, 18)
BIG = ((5 << 32) + 17, (3 << 32) + 9)   # a seed and an offset above 2^32
CASES = [lambda TQ, TK: (TK + 1, 1, -1), lambda TQ, TK: (TQ + 1, 5, 0), lambda TQ, TK: (2 * TQ + 3, 5, 2),
         lambda TQ, TK: (2 * TQ + 3, TK, 1), lambda TQ, TK: (2 * TQ + 3, TK + 8, -1)]
SMALL = {'encoder.num_units': 64, 'encoder.num_heads': 2, 'encoder.ff_units': 96, 'encoder.num_layers': 2,
         'encoder.conv_channels': '32 32', 'encoder.feature_blocks': 3, 'trainer.batch_size': 3}
IDS = ['causal', 'own-chunk', 'C5-L2', 'C=TK-L1', 'C=TK+8-all']


def raw(precision, q_dev, ld, len_dev, H, dk, extra, do_dev=None, o=None, lse=None):
    """the win entry points into guarded buffers: forward [o, lse] or, given do, [dqkv]; extra = (keep, seed, offset, C, Lc)"""
    B, T = q_dev.shape[:2]
    fn = getattr(_hip.lib(), 'nabu_self_attn_%swin_%s' % ('bf16_' if precision == 'bf16' else '', 'fwd' if do_dev is None else 'bwd'))
    outs = [guarded((B, T, H * dk)), guarded((B, H, T))] if do_dev is None else [guarded((B, T, ld))]
    mid = [] if do_dev is None else [_hip.ptr(o.contiguous()), _hip.ptr(lse.contiguous()), _hip.ptr(do_dev)]
    _hip.check(fn(B, T, H, dk, _hip.ptr(q_dev), ld, *mid, _hip.ptr(len_dev), *extra, *(v.data_ptr() for _, v in outs), _hip.stream()), 'win')
    assert all(clean(buf) for buf, _ in outs)
    return [v for _, v in outs]


def against_float64(precision, dk, H, T, C, Lc, drop):
    """o, lse, dq, dk, dv each: ||got - ref||inf <= FACTOR ||restatement - ref||inf; ref = float64 attn_*_win, restatement =
    the same in float32 (f32) or with (d . P) and dS rounded to bf16 (bf16, inputs rounded before upload).  Rows >= len are
    +0.0 by bits; spare columns and guards untouched; no NaN or inf; two backward calls give equal bits."""
    rng = np.random.default_rng(dk * 1000 + H * 10 + T + C)
    D, ld, low = H * dk, 3 * H * dk + 4, precision == 'bf16'
    lens = np.array([T, 0, 1, min(C, T), T - 1], np.int32)
    qkv, do = rng.standard_normal((5, T, ld)).astype(np.float32), rng.standard_normal((5, T, D)).astype(np.float32)
    if low:
        qkv, do = bf16_rne(qkv)[1], bf16_rne(do)[1]
    q_dev, len_dev, do_dev, extra = dev(qkv), dev(lens, np.int32), dev(do), drop + (C, Lc)
    o, lse = raw(precision, q_dev, ld, len_dev, H, dk, extra)
    got = [raw(precision, q_dev, ld, len_dev, H, dk, extra, do_dev, o, lse)[0].cpu().numpy() for _ in range(2)]
    np.testing.assert_array_equal(got[0].view(np.int32), got[1].view(np.int32))
    assert np.all(got[0][:, :, 3 * D:] == SENTINEL)
    q3, d = qkv[:, :, :3 * D], None if drop[0] == 1 else keep_scale(5, H, T, *drop)
    ref_o, ref_lse = attn_fwd_win(q3, lens, H, (C, Lc), d)
    low_o, low_lse = attn_fwd_win(q3, lens, H, (C, Lc), d, np.float32, low)
    ref = attn_bwd_win(q3, ref_o, ref_lse, do, lens, H, (C, Lc), d)
    low_g = attn_bwd_win(q3, low_o, low_lse, do, lens, H, (C, Lc), d, np.float32, low)
    figures = [('o', o.cpu().numpy(), ref_o, low_o), ('lse', *(a.transpose(0, 2, 1) for a in (lse.cpu().numpy(), ref_lse, low_lse)))]
    figures += [(n, *(a[:, :, i * D:(i + 1) * D] for a in (got[0], ref, low_g))) for i, n in enumerate(('dq', 'dk', 'dv'))]
    for name, g, r, f in figures:
        err, floor = np.abs(g - r).max(), np.abs(f - r).max()
        print(precision, name, 'error / floor %.3f' % (err / floor))
        assert np.all(np.isfinite(g)) and err <= FACTOR[precision] * floor, (name, err / floor)
        assert all(np.all(np.ascontiguousarray(g[b, L:]).view(np.int32) == 0) for b, L in enumerate(lens)), name


@pytest.mark.parametrize('which', range(5), ids=IDS)
@pytest.mark.parametrize('dk', [32, 64])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_forward_and_backward_against_float64(precision, dk, which):
    """a first walked tile that is not tile 0, a window starting mid-tile, chunk edges off tile edges, lanes whose first
    walked tiles hold nothing they see, dK/dV workgroups whose query range ends before len.  Largest ratios measured
    (DESIGN.md section 19): 3.29 (f32, at dq) and 1.80 (bf16, at lse)."""
    T, C, Lc = CASES[which](*hip.self_attn_tiles(precision))
    against_float64(precision, dk, 3 if which == 2 else 1, T, C, Lc, (1.0, 0, 0))


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_dropout_under_a_window_against_float64(precision):
    """keep 0.9 at (2 TQ + 3, 5, 2): the reference carries both masks"""
    T, C, Lc = CASES[2](*hip.self_attn_tiles(precision))
    against_float64(precision, 64, 2, T, C, Lc, (0.9,) + BIG)


def run(precision, x, d, lens, H, window):
    """[o, lse^T, dqkv] (all [B,T,.]) through ops.self_attn_fwd / _bwd"""
    o, lse = hip.self_attn_fwd(dev(x), dev(lens, np.int32), H, precision, window=window)
    dqkv = hip.self_attn_bwd(dev(x), o, lse, dev(d), dev(lens, np.int32), H, precision, window=window)
    return [t.cpu().numpy() for t in (o, lse.transpose(1, 2), dqkv)]


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_the_exact_properties(precision):
    """bit for bit.  C >= T with Lc = -1 is the plain call, forward and backward.  Prefix: with Lc = -1 rows < c C of o and
    lse at length L are those of the same data at length c C (off a tile edge).  Padding: the utterance alone at T = L, or
    inside T = 2 TQ + 9 with 1e30 in the padding rows, gives the same o, lse and dqkv, and rows >= len are +0.0."""
    TQ, TK = hip.self_attn_tiles(precision)
    rng = np.random.default_rng(5)
    H, dk, L, T, C = 2, 64, TQ + TK + 5, 2 * TQ + 9, 7
    D, cC = H * dk, 7 * (TK // 7 + 2)                                                    # TK < c C < 2 TK, no multiple of TK
    qkv = np.full((2, T, 3 * D), 1e30, np.float32)
    qkv[:, :L] = rng.standard_normal((2, L, 3 * D))
    do = rng.standard_normal((2, T, D)).astype(np.float32)
    plain = run(precision, qkv[:, :L], do[:, :L], [L, L - 3], H, None)
    for a, b in zip(run(precision, qkv[:, :L], do[:, :L], [L, L - 3], H, (L + 7, -1)), plain):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    whole, prefix = run(precision, qkv, do, [L, L], H, (C, -1)), run(precision, qkv, do, [cC, cC], H, (C, -1))
    for a, b in zip(whole[:2], prefix[:2]):
        np.testing.assert_array_equal(a[:, :cC].view(np.int32), b[:, :cC].view(np.int32))
    inside, alone = run(precision, qkv, do, [L, T], H, (16, 2)), run(precision, qkv[:1, :L], do[:1, :L], [L], H, (16, 2))
    for a, b in zip(inside, alone):
        np.testing.assert_array_equal(a[0, :L].view(np.int32), b[0].view(np.int32))
        assert np.all(a[0, L:].view(np.int32) == 0)
    assert np.any(inside[0][0, :L] != plain[0][0])                                       # (and the window is there)


def test_the_keys_reach_the_kernel():
    """transformer_ctc with both keys through the recipe API (8 pooled frames): a finite loss, other bits than without them"""
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)
    batch, losses = data.batch(0), []
    for keys in ({'encoder.attention_chunk': 4, 'encoder.attention_left_chunks': 1}, {}):
        ops.set_seed(0)
        mc, tc, ec = recipes.load_recipe('transformer_ctc', **SMALL, **keys)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None, server=None, task_index=0)
        losses.append(tr.step(tr.to_device(batch)).cpu().numpy().reshape(-1)[0])
    assert np.isfinite(losses[0]) and losses[0].view(np.int32) != losses[1].view(np.int32)


def test_one_block_through_the_tape(monkeypatch):
    """tests/test_hip_self_attn.py's block test with attention_window=(2, 1) and the windowed attention in the float64 block"""
    block = layer.self_attention_block
    monkeypatch.setattr(layer, 'self_attention_block', lambda *args, **kw: block(*args, attention_window=(2, 1), **kw))
    monkeypatch.setattr(R, 'attn_fwd', lambda qkv, lens, H: attn_fwd_win(qkv, lens, H, (2, 1)))
    monkeypatch.setattr(R, 'attn_bwd', lambda *args: attn_bwd_win(*args, (2, 1)))
    plain_tests.test_one_block_through_the_tape()
