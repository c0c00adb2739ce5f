"""GPU: self_attn_bf16.hip (attention_precision = bf16) against the float64 restatement of tests/self_attn_ref.py, at the
shapes of tests/test_hip_self_attn.py placed around ITS tiles (k = 64 streamed, q = 128 owned).  Inputs are rounded to bf16
before upload, so the reference sees the operands the matrix unit sees and only P's and dS's roundings are internal."""
import numpy as np
import pytest

from nabu_amd import _hip, ops as hip
from nabu_amd.neuralnetworks.components import ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import self_attn_ref as R
from tests.gemm_pk_cases import bf16_rne
from tests.self_attn_bf16_ref import attn_bwd_bf16
from tests.test_hip_self_attn import SENTINEL, U, clean, dev, guarded, make_trainer

pytestmark = pytest.mark.gpu
TQ, TK = 128, 64                        # nabu_self_attn_bf16_tile_q / _k (asserted below)
TS = [1, TK - 1, TK, TK + 1, TQ + 1, 2 * max(TQ, TK) + 3, 301]
U16 = 2.0 ** -8
BWD_FACTOR = 4.0                        # the next power of two above twice the measured 1.27


def batch(rng, T, H, dk, regime='normal'):
    """test_hip_self_attn.batch with this file's TK, rounded to bf16: (qkv [5,T,3D+4], lens)"""
    D = H * dk
    lens = np.clip(np.array([T, 0, 1, TK, T - 1]), 0, T).astype(np.int32)
    qkv = rng.standard_normal((5, T, 3 * D + 4)).astype(np.float32)
    if regime == 'equal':
        qkv[:, :, D:2 * D] = qkv[:, :1, D:2 * D]
    if regime == 'spread':
        qkv[:, :, :2 * D] *= np.float32(np.sqrt(1e4 / 3.0))
    return bf16_rne(qkv)[1], lens


def raw_bwd(q_dev, ld, o, lse, do_dev, len_dev, H, dk):
    """nabu_self_attn_bf16_bwd into a guarded buffer at row stride ld: (dqkv [B,T,ld], guards untouched)"""
    B, T = do_dev.shape[:2]
    buf, dqkv = guarded((B, T, ld))
    _hip.check(_hip.lib().nabu_self_attn_bf16_bwd(B, T, H, dk, _hip.ptr(q_dev), ld, _hip.ptr(o), _hip.ptr(lse), _hip.ptr(do_dev),
                                                  _hip.ptr(len_dev), dqkv.data_ptr(), _hip.stream()), 'bwd')
    return dqkv.cpu().numpy(), clean(buf)


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('H', [1, 3])
@pytest.mark.parametrize('dk', [32, 64])
def test_forward_within_the_derived_bound(dk, H, T):
    """|o - ref| <= ((1 + u16) exp(2 E) (1 + gamma(L + c2)) - 1) A componentwise: the fp32 kernel's bound (E, A, c2 and the
    measured eps as in tests/test_hip_self_attn.py, with this kernel's tile of 64 keys) times ONE bf16 rounding of each
    probability, u16 = 2^-8; Q, K and V round to themselves.  lse sees no 16-bit rounding and keeps the fp32 bound.
    Rows >= len are +0.0 bit for bit, the guards untouched, no NaN or inf."""
    assert hip.self_attn_tiles('bf16') == (TQ, TK)
    rng = np.random.default_rng(dk * 1000 + H * 10 + T)
    for regime in ('normal', 'equal', 'spread'):
        qkv, lens = batch(rng, T, H, dk, regime)
        (bo, o), (bl, lse) = guarded((5, T, H * dk)), guarded((5, H, T))
        q_dev, len_dev = dev(qkv), dev(lens, np.int32)
        _hip.check(_hip.lib().nabu_self_attn_bf16_fwd(5, T, H, dk, _hip.ptr(q_dev), 3 * H * dk + 4, _hip.ptr(len_dev),
                                                      o.data_ptr(), lse.data_ptr(), _hip.stream()), 'fwd')
        o, lse = o.cpu().numpy(), lse.cpu().numpy()
        q3 = qkv[:, :, :3 * H * dk]
        ro, rl, E, A = R.attn_fwd(q3, lens, H, bound=True)
        fo, _ = R.attn_fwd(q3, lens, H, dtype=np.float32)
        eps = float(np.max(np.abs(fo - ro) / np.maximum(A, 1e-300))) / U
        Lr = np.clip(lens, 0, T).astype(np.float64)[:, None, None]
        c2 = Lr + 3 * np.ceil(Lr / TK) + 1 + 2 * (np.ceil(Lr / TK) + 1) * 2 * eps
        Eg = R.gamma(dk + 2) * E                                             # [B,H,T]; repeated over dk: [B,T,D]
        bound = ((1 + U16) * np.exp(2 * np.repeat(Eg.transpose(0, 2, 1), dk, axis=2)) * (1 + R.gamma(Lr + c2)) - 1) * A
        lb = np.expm1(Eg) + R.gamma(c2 + 4) * (1 + np.abs(rl) + E)
        print(regime, 'o: error / bound %.3g' % np.max(np.abs(o - ro) / np.maximum(bound, 1e-300)),
              'lse: %.3g' % np.max(np.abs(lse - rl) / lb))
        assert clean(bo) and clean(bl) and np.all(np.isfinite(o)) and np.all(np.isfinite(lse)), regime
        assert np.all(np.abs(o - ro) <= bound), regime
        assert np.all(np.abs(lse - rl) <= lb), (regime, float(np.max(np.abs(lse - rl) - lb)))
        for b, L in enumerate(lens):
            assert np.all(o[b, L:].view(np.int32) == 0) and np.all(lse[b, :, L:].view(np.int32) == 0), (regime, b)


@pytest.mark.parametrize('T', [TK - 1, TK + 1, TQ + 1, 2 * max(TQ, TK) + 3])
@pytest.mark.parametrize('H', [1, 3])
@pytest.mark.parametrize('dk', [32, 64])
def test_backward_at_the_floor_of_its_restatement(dk, H, T):
    """dq, dk, dv each: ||got - ref||inf <= BWD_FACTOR ||restatement - ref||inf, ref = float64 attn_bwd on the rounded
    inputs, restatement = self_attn_bf16_ref.attn_bwd_bf16 (float32, P and dS rounded where the kernels round them).  The
    fused order adds one rounding per key tile and nothing more; the largest ratio measured is 1.27, twice that lies below
    4, so the factor is 4.  Rows >= len are +0.0, the spare columns and the guards untouched, two calls give equal bits."""
    rng = np.random.default_rng(dk * 1000 + H * 10 + T)
    qkv, lens = batch(rng, T, H, dk)
    D, ld = H * dk, 3 * H * dk + 4
    do = bf16_rne(rng.standard_normal((5, T, D)).astype(np.float32))[1]
    q_dev, len_dev, do_dev = dev(qkv), dev(lens, np.int32), dev(do)
    o, lse = hip.self_attn_fwd(q_dev[:, :, :3 * D], len_dev, H, 'bf16')
    got, ok = raw_bwd(q_dev, ld, o, lse, do_dev, len_dev, H, dk)
    again, ok2 = raw_bwd(q_dev, ld, o, lse, do_dev, len_dev, H, dk)
    assert ok and ok2 and np.all(got[:, :, 3 * D:] == SENTINEL)
    np.testing.assert_array_equal(got.view(np.int32), again.view(np.int32))
    q3 = qkv[:, :, :3 * D]
    ref = R.attn_bwd(q3, *R.attn_fwd(q3, lens, H), do, lens, H)
    low = attn_bwd_bf16(q3, R.attn_fwd(q3, lens, H, dtype=np.float32)[1], do, lens, H)
    for i, name in enumerate(('dq', 'dk', 'dv')):
        g, r, f = (a[:, :, i * D:(i + 1) * D] for a in (got, ref, low))
        err, floor = np.abs(g - r).max(), np.abs(f - r).max()
        print(name, 'error / floor %.3f' % (err / floor))
        assert err <= BWD_FACTOR * floor, (name, err / floor)
        assert all(np.all(g[b, L:].view(np.int32) == 0) for b, L in enumerate(lens)), name


def test_the_rounding_is_round_to_nearest_even():
    """N(0,1) qkv that bf16 does not hold gives the bits of bf16_rne(qkv), forward and backward (o and lse of the same
    forward call); do that bf16 does not hold gives dv the bits of bf16_rne(do) — dq and dk see the fp32 do through
    delta = rowsum(do . o), so they are compared at the same do."""
    rng = np.random.default_rng(5)
    H, dk, T = 2, 64, TK + 5
    D = H * dk
    qkv, do = rng.standard_normal((2, T, 3 * D)).astype(np.float32), rng.standard_normal((2, T, D)).astype(np.float32)
    len_dev, res = dev([T, T - 3], np.int32), []
    assert np.any(bf16_rne(qkv)[1] != qkv)
    for x, d in ((qkv, do), (bf16_rne(qkv)[1], do), (bf16_rne(qkv)[1], bf16_rne(do)[1])):
        o, lse = hip.self_attn_fwd(dev(x), len_dev, H, 'bf16')
        res.append([t.cpu().numpy().view(np.int32) for t in (o, lse, hip.self_attn_bwd(dev(x), o, lse, dev(d), len_dev, H, 'bf16'))])
    for a, b in zip(res[0], res[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res[0][2][:, :, 2 * D:], res[2][2][:, :, 2 * D:])


@pytest.mark.parametrize('dk', [32, 64])
def test_an_utterance_does_not_see_its_padding(dk):
    """alone at T = len, or inside a longer batch whose padding rows of qkv hold 1e30: o, lse and dqkv are the same bits"""
    rng = np.random.default_rng(3)
    H, L, T = 2, TQ + TK + 5, 2 * TQ + 9
    D = H * dk
    qkv = np.full((2, T, 3 * D), 1e30, np.float32)
    qkv[0, :L] = rng.standard_normal((L, 3 * D))
    do = rng.standard_normal((2, T, D)).astype(np.float32)
    res = []
    for x, d, lens in ((qkv, do, [L, T]), (qkv[:1, :L], do[:1, :L], [L])):
        o, lse = hip.self_attn_fwd(dev(x), dev(lens, np.int32), H, 'bf16')
        dqkv = hip.self_attn_bwd(dev(x), o, lse, dev(d), dev(lens, np.int32), H, 'bf16')
        res.append([t.cpu().numpy() for t in (o, lse.transpose(1, 2), dqkv)])            # all [B, T, .]
    for inside, alone in zip(*res):
        np.testing.assert_array_equal(inside[0, :L].view(np.int32), alone[0].view(np.int32))
        assert np.all(inside[0, L:] == 0)


@pytest.mark.parametrize('encoder', ['transformer', 'conformer'])
def test_the_key_reaches_the_kernel(encoder):
    """encoder.attention_precision = bf16 through the recipe API: a finite loss, the same bits from the same seed, and
    other bits than the f32 run of the same seed and batch (the relative distance is printed, not gated: DESIGN.md)"""
    over = {'encoder.encoder': encoder, 'encoder.conv_kernel': 7} if encoder == 'conformer' else {}
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)
    raw, losses = data.batch(0), []
    for precision in ('bf16', 'bf16', 'f32'):
        ops.set_seed(0)
        tr = make_trainer(data, **dict(over, **{'encoder.attention_precision': precision}))
        losses.append(tr.step(tr.to_device(raw)).cpu().numpy().reshape(-1)[0])
    print(encoder, 'loss bf16 %.7g, f32 %.7g, relative distance %.3g' % (losses[0], losses[2], abs(losses[0] - losses[2]) / abs(losses[2])))
    assert np.isfinite(losses[0]) and losses[0].view(np.int32) == losses[1].view(np.int32)
    assert losses[0].view(np.int32) != losses[2].view(np.int32)
