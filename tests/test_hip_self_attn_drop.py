"""GPU: dropout on the attention probabilities inside the self-attention kernels (nabu_self_attn[_bf16]_drop_*) against
the float64 restatement of tests/self_attn_drop_ref.py, whose mask comes from the host Philox (oracle/philox.py)."""
import numpy as np
import pytest
import torch

import tests.test_hip_self_attn as plain_tests
from nabu_amd import _hip, ops as hip
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import self_attn_ref as R
from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_drop_ref import attn_bwd_drop, attn_fwd_drop, keep_scale
from tests.test_hip_self_attn import SENTINEL, clean, dev, guarded, make_trainer

pytestmark = pytest.mark.gpu
FACTOR = {'f32': 8.0, 'bf16': 4.0}      # see test_forward_and_backward_against_float64
BIG = ((5 << 32) + 17, (3 << 32) + 9)   # a seed and an offset above 2^32: the high key and counter words count


def raw(precision, q_dev, ld, len_dev, H, dk, drop, do_dev=None, o=None, lse=None):
    """the drop entry points into guarded buffers at row stride ld: forward [o, lse] or, given do, backward [dqkv]"""
    B, T = q_dev.shape[:2]
    fn = getattr(_hip.lib(), 'nabu_self_attn_%sdrop_%s' % ('bf16_' if precision == 'bf16' else '', 'fwd' if do_dev is None else 'bwd'))
    outs = [guarded((B, T, H * dk)), guarded((B, H, T))] if do_dev is None else [guarded((B, T, ld))]
    mid = [] if do_dev is None else [_hip.ptr(o.contiguous()), _hip.ptr(lse.contiguous()), _hip.ptr(do_dev)]
    _hip.check(fn(B, T, H, dk, _hip.ptr(q_dev), ld, *mid, _hip.ptr(len_dev), *drop, *(v.data_ptr() for _, v in outs), _hip.stream()), 'drop')
    assert all(clean(buf) for buf, _ in outs)
    return [v for _, v in outs]


@pytest.mark.parametrize('drop', [(0.5, 1234, 77), (0.9,) + BIG], ids=['keep0.5', 'keep0.9'])
@pytest.mark.parametrize('which', range(4), ids=['TK-1', 'TK+1', 'TQ+1', '2max+3'])
@pytest.mark.parametrize('H', [1, 3])
@pytest.mark.parametrize('dk', [32, 64])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_forward_and_backward_against_float64(precision, dk, H, which, drop):
    """o, dq, dk, dv each: ||got - ref||inf <= FACTOR ||restatement - ref||inf; ref = float64 attn_*_drop, restatement =
    the same in float32 (f32) or in float32 with (d . P) and dS rounded to bf16 (bf16, inputs rounded before upload).
    FACTOR is the next power of two above twice the largest ratio measured over all cases:
    3.24 (f32, at o; dq 2.00, dk 2.57, dv 3.16) and 1.17 (bf16, at dk); the plain kernels' figures are 2.16 and 1.27, and
    the mask adds one multiply per probability.  lse is the plain kernel's bit for bit; rows >= len are +0.0 by bits; spare
    columns and guards are untouched; no NaN or inf (len 1 at keep 0.5 has empty kept sets); two backward calls give
    equal bits.  Lengths [T, 0, 1, TK, T - 1] around the precision's own tiles, row stride 3 D + 4."""
    TQ, TK = hip.self_attn_tiles(precision)
    T = [TK - 1, TK + 1, TQ + 1, 2 * max(TQ, TK) + 3][which]
    rng = np.random.default_rng(dk * 1000 + H * 10 + T)
    D, ld, low = H * dk, 3 * H * dk + 4, precision == 'bf16'
    lens = np.array([T, 0, 1, TK, T - 1], np.int32)
    qkv, do = rng.standard_normal((5, T, ld)).astype(np.float32), rng.standard_normal((5, T, D)).astype(np.float32)
    if low:
        qkv, do = bf16_rne(qkv)[1], bf16_rne(do)[1]
    q_dev, len_dev, do_dev = dev(qkv), dev(lens, np.int32), dev(do)
    o, lse = raw(precision, q_dev, ld, len_dev, H, dk, drop)
    assert torch.equal(lse.view(torch.int32), hip.self_attn_fwd(q_dev[:, :, :3 * D], len_dev, H, precision)[1].view(torch.int32))
    got = [raw(precision, q_dev, ld, len_dev, H, dk, drop, do_dev, o, lse)[0].cpu().numpy() for _ in range(2)]
    np.testing.assert_array_equal(got[0].view(np.int32), got[1].view(np.int32))
    assert np.all(got[0][:, :, 3 * D:] == SENTINEL)
    q3, d = qkv[:, :, :3 * D], keep_scale(5, H, T, *drop)
    ref_o, ref_lse = attn_fwd_drop(q3, lens, H, d)
    low_o, low_lse = attn_fwd_drop(q3, lens, H, d, np.float32, low)
    ref, low_g = attn_bwd_drop(q3, ref_o, ref_lse, do, lens, H, d), attn_bwd_drop(q3, low_o, low_lse, do, lens, H, d, np.float32, low)
    for name, g, r, f in [('o', o.cpu().numpy(), ref_o, low_o)] + [(n, *(a[:, :, i * D:(i + 1) * D] for a in (got[0], ref, low_g)))
                                                                    for i, n in enumerate(('dq', 'dk', 'dv'))]:
        err, floor = np.abs(g - r).max(), np.abs(f - r).max()
        print(name, 'error / floor %.3f' % (err / floor))
        assert np.all(np.isfinite(g)) and err <= FACTOR[precision] * floor, (name, err / floor)
        assert all(np.all(g[b, L:].view(np.int32) == 0) for b, L in enumerate(lens)), name
    lse = lse.cpu().numpy()
    assert np.all(np.isfinite(lse)) and all(np.all(lse[b, :, L:].view(np.int32) == 0) for b, L in enumerate(lens))


def run(precision, x, d, lens, H, keep=1.0, rng=None):
    """[o, lse^T, dqkv] (all [B,T,.]) through ops.self_attn_fwd / _bwd"""
    o, lse = hip.self_attn_fwd(dev(x), dev(lens, np.int32), H, precision, keep, rng)
    dqkv = hip.self_attn_bwd(dev(x), o, lse, dev(d), dev(lens, np.int32), H, precision, keep, rng)
    return [t.cpu().numpy() for t in (o, lse.transpose(1, 2), dqkv)]


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_keep_one_is_the_plain_path_and_the_mask_does_not_depend_on_padding_or_T(precision):
    """keep = 1 through the _drop_ entry points: o, lse and dqkv are the plain entry points' bits.  keep 0.75, one (seed,
    offset): row 0 alone at T = L, or inside T = 2 TQ + 9 with 1e30 in the padding, gives the same bits of all three"""
    TQ, TK = hip.self_attn_tiles(precision)
    rng = np.random.default_rng(3)
    H, dk, L, T = 2, 64, TQ + TK + 5, 2 * TQ + 9
    D = H * dk
    qkv = np.full((2, T, 3 * D), 1e30, np.float32)
    qkv[:, :L] = rng.standard_normal((2, L, 3 * D))
    do = rng.standard_normal((2, T, D)).astype(np.float32)
    q_dev, len_dev, plain = dev(qkv[:, :L]), dev([L, L - 3], np.int32), run(precision, qkv[:, :L], do[:, :L], [L, L - 3], H)
    o, lse = raw(precision, q_dev, 3 * D, len_dev, H, dk, (1.0,) + BIG)
    dqkv, = raw(precision, q_dev, 3 * D, len_dev, H, dk, (1.0,) + BIG, dev(do[:, :L]), o, lse)
    for a, b in zip((o, lse.transpose(1, 2), dqkv), plain):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32))
    inside, alone = run(precision, qkv, do, [L, T], H, 0.75, BIG), run(precision, qkv[:1, :L], do[:1, :L], [L], H, 0.75, BIG)
    for a, b in zip(inside, alone):
        np.testing.assert_array_equal(a[0, :L].view(np.int32), b[0].view(np.int32))
        assert np.all(a[0, L:] == 0)
    assert np.any(inside[0][0, :L] != plain[0][0])                                      # (and the mask is there)


@pytest.mark.parametrize('encoder', ['transformer', 'conformer'])
def test_the_key_reaches_the_kernel(encoder):
    """encoder.attention_dropout = 0.8 through the recipe API: a finite loss, the same bits from the same seed, other bits
    than the run without the key; attention_dropout = 1.0 gives the bits of the run without the key"""
    over = {'encoder.encoder': encoder, 'encoder.conv_kernel': 7} if encoder == 'conformer' else {}
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)
    batch, losses = data.batch(0), []
    for value in (0.8, 0.8, None, 1.0):
        ops.set_seed(0)
        tr = make_trainer(data, **dict(over, **({} if value is None else {'encoder.attention_dropout': value})))
        losses.append(tr.step(tr.to_device(batch)).cpu().numpy().reshape(-1)[0].view(np.int32))
    assert np.isfinite(losses[0].view(np.float32)) and losses[0] == losses[1] and losses[0] != losses[2] and losses[2] == losses[3]


def test_one_block_through_the_tape(monkeypatch):
    """tests/test_hip_self_attn.py's block test (B 3, T 9, D 64, H 2, lens [9, 4, 0], 2e-4 of the largest entry) with
    layer.self_attention_block(keep=1, attention_keep=0.7) and the masked attention in the float64 block's place; the mask
    comes from the ONE draw the taped call took: the stream's offset is recorded before each call and replayed"""
    block, before = layer.self_attention_block, []

    def dropped(*args, **kw):
        before.append(ops.global_rng().offset)
        return block(*args, attention_keep=0.7, **kw)

    def mask():
        assert before[0] == before[1] == ops.global_rng().offset - 1                    # no draw without a tape, one under it
        return keep_scale(3, 2, 9, 0.7, ops.global_rng().seed, before[1] + 1)
    monkeypatch.setattr(layer, 'self_attention_block', dropped)
    monkeypatch.setattr(R, 'attn_fwd', lambda qkv, lens, H: attn_fwd_drop(qkv, lens, H, mask()))
    monkeypatch.setattr(R, 'attn_bwd', lambda *args: attn_bwd_drop(*args, mask()))
    plain_tests.test_one_block_through_the_tape()
