"""GPU: conv_module.hip, the Swish kernels, layer.conformer_block and `encoder = conformer` against the torch CPU
restatement (tests/conformer_ref.py) in float64, at the smallest shapes that reach every branch: all three tap classes,
one and two channel chunks (and the LDS limit), sizes around the owned tile, lengths 0 .. T in every batch, a row stride
with spare columns.

The yardstick of every tensor: ||got - ref64||inf <= 8 max(||ref32 - ref64||inf, 2^-24 ||ref64||inf), where ref32 is the
restatement in float32 — the reference's own rounding floor, computed from the reference alone.  8 is the project's
margin for a fused kernel against such a floor (BWD_FACTOR of tests/test_hip_self_attn.py): the fused order differs from
the restatement's by fma contraction, the moments' tree and the workgroups' partial sums, none of which lengthens a
rounding chain.  A ratio above 8 is a defect.  Each test prints its ratios (DESIGN.md section 16 has the largest)."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip, ops as hip
from nabu_amd.autodiff import Tape, record
from nabu_amd import variables as vs
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import conformer_ref as R
from tests.test_hip_self_attn import SENTINEL, clean, dev, guarded, make_trainer

pytestmark = pytest.mark.gpu
U, FACTOR = 2.0 ** -24, 8.0
TT = 32                                  # nabu_conv_module_tile_t (asserted below)


def within(name, got, ref64, ref32):
    floor = max(np.abs(ref32 - ref64).max(), U * np.abs(ref64).max())
    err = np.abs(got - ref64).max()
    print('%s: %.3f of the floor' % (name, err / floor))
    assert np.all(np.isfinite(got)) and err <= FACTOR * floor, (name, err / floor)


def operands(rng, K, D):
    return [a.astype(np.float32) for a in (rng.standard_normal((K, D)) / np.sqrt(K), 0.1 * rng.standard_normal(D),
                                           1 + 0.1 * rng.standard_normal(D), 0.1 * rng.standard_normal(D))]


def fused(u, lens, par, dy, K, D):
    """both entry points into guarded buffers: ({name: array} as conformer_ref.CORE plus mean, rstd; guards untouched)"""
    B, T, ld = u.shape
    L = _hip.lib()
    u_d, len_d, dy_d, par_d = dev(u), dev(lens, np.int32), dev(dy), [dev(p) for p in par]
    (by, y), (bm, mean), (br, rstd) = guarded((B, T, D)), guarded((B, T)), guarded((B, T))
    _hip.check(L.nabu_conv_module_fwd(B, T, D, K, _hip.ptr(u_d), ld, _hip.ptr(len_d), *[_hip.ptr(p) for p in par_d], layer.LN_EPS,
                                      y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _hip.stream()), 'fwd')
    parts = L.nabu_conv_module_parts(B, T)
    (bu, du), (bz, dz), (bl, pl), (bw, pw) = guarded((B, T, ld)), guarded((B, T, D)), guarded((parts, 3 * D)), guarded((parts, K * D))
    _hip.check(L.nabu_conv_module_bwd(B, T, D, K, _hip.ptr(u_d), ld, _hip.ptr(len_d), *[_hip.ptr(p) for p in par_d],
                                      mean.data_ptr(), rstd.data_ptr(), _hip.ptr(dy_d), du.data_ptr(), dz.data_ptr(),
                                      pl.data_ptr(), pw.data_ptr(), _hip.stream()), 'bwd')
    ln = hip.colsum(pl, torch.empty(3 * D, device='cuda')).cpu().numpy()
    out = {'y': y, 'mean': mean, 'rstd': rstd, 'du': du, 'dw': hip.colsum(pw, torch.empty(K * D, device='cuda')).view(K, D)}
    out = dict({n: t.cpu().numpy() for n, t in out.items()}, dgamma=ln[:D], dbeta=ln[D:2 * D], dbw=ln[2 * D:])
    return out, all(clean(b) for b in (by, bm, br, bu, bz, bl, bw))


CASES = [(K, D, T) for K in (3, 15, 31) for D in (64, 320) for T in (1, TT - 1, TT + 1, 2 * TT + K)] + [(31, 1024, TT + 1)]


@pytest.mark.parametrize('K,D,T', CASES)
def test_the_core_against_float64(K, D, T):
    """y, du, dw, dbw, dgamma, dbeta within the yardstick; rows >= len of y, mean, rstd and du +0.0 bit for bit; spare
    columns and guards untouched; two backward calls give equal bits"""
    assert hip.conv_module_tile_t() == TT
    rng = np.random.default_rng(K * 10000 + D * 10 + T)
    lens = np.array([T, 0, 1, min((K - 1) // 2, T), T - 1], np.int32)
    u = np.full((5, T, 2 * D + 4), SENTINEL, np.float32)
    u[:, :, :2 * D] = rng.standard_normal((5, T, 2 * D))
    par, dy = operands(rng, K, D), rng.standard_normal((5, T, D)).astype(np.float32)
    got, ok = fused(u, lens, par, dy, K, D)
    again, ok2 = fused(u, lens, par, dy, K, D)
    assert ok and ok2 and np.all(got['du'][:, :, 2 * D:] == SENTINEL)
    for n in got:
        np.testing.assert_array_equal(got[n].view(np.int32), again[n].view(np.int32), err_msg=n)
    for b, L in enumerate(lens):
        assert all(np.all(got[n][b, L:].view(np.int32) == 0) for n in ('y', 'mean', 'rstd')), b
        assert np.all(got['du'][b, L:, :2 * D].view(np.int32) == 0), b
    ref64 = R.conv_module(u[:, :, :2 * D], lens, *par, dy)
    ref32 = R.conv_module(u[:, :, :2 * D], lens, *par, dy, dtype=torch.float32)
    for n in R.CORE:
        within(n, got[n][:, :, :2 * D] if n == 'du' else got[n], ref64[n], ref32[n])


@pytest.mark.parametrize('K', [3, 31])
def test_an_utterance_does_not_see_its_padding(K):
    """alone at T = len, or inside a longer batch whose padding rows of u hold 1e30 and whose other row is empty: y, du,
    dw and dgamma are the same bits"""
    rng = np.random.default_rng(K)
    D, L, T = 64, TT + K, 2 * TT + 9
    u = np.full((2, T, 2 * D), 1e30, np.float32)
    u[0, :L] = rng.standard_normal((L, 2 * D))
    par, dy = [dev(p) for p in operands(rng, K, D)], rng.standard_normal((2, T, D)).astype(np.float32)
    res = []
    for x, d, lens in ((u, dy, [L, 0]), (u[:1, :L], dy[:1, :L], [L])):
        y, mean, rstd = hip.conv_module_fwd(dev(x), dev(lens, np.int32), *par, layer.LN_EPS)
        du, dw, _, dgamma, _ = hip.conv_module_bwd(dev(x), dev(lens, np.int32), *par, mean, rstd, dev(d))
        res.append([t.cpu().numpy() for t in (y, du, dw, dgamma)])
    (y, du, dw, dgamma), alone = res
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(du)) and np.all(y[:, L:] == 0) and np.all(du[:, L:] == 0)
    for inside, single in ((y[0, :L], alone[0][0]), (du[0, :L], alone[1][0]), (dw, alone[2]), (dgamma, alone[3])):
        np.testing.assert_array_equal(inside.view(np.int32), single.view(np.int32))


def test_swish_and_its_gradient():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-30, 30, 994), [0.0, -0.0, 88.0, -88.0, 30.0, -30.0]]).astype(np.float32)
    dy = rng.standard_normal(1000).astype(np.float32)
    (y64, dx64), (y32, dx32) = R.swish(x, dy), R.swish(x, dy, torch.float32)
    within('swish', hip.swish(dev(x)).cpu().numpy(), y64, y32)
    within('swish_bwd', hip.swish_bwd(dev(x), dev(dy)).cpu().numpy(), dx64, dx32)


def test_one_block_through_the_tape():
    """layer.conformer_block under a tape at gemm_precision f32, input taped: the output, dh and every parameter
    gradient against the float64 block, with the block yardstick of test_hip_self_attn.py (2e-4 of the largest entry)"""
    rng = np.random.default_rng(12)
    B, T, D, H, FF, K = 3, 9, 64, 2, 128, 7
    lens, x = np.array([9, 4, 0], np.int32), rng.standard_normal((B, T, D)).astype(np.float32)
    store, got, layer.GEMM_PRECISION[0] = vs.VariableStore(seed=4), [], 'f32'
    with vs.as_default(store):
        layer.conformer_block(dev(x), dev(lens, np.int32), H, FF, K, scope='blk')       # creates the variables
        for n in R.NAMES:
            if n.endswith(('biases', 'bias', 'beta')):
                store.vars['blk/' + n].data.normal_()              # (they start at zero: make them count)
        with Tape() as tape:
            xin = dev(x)
            record([dev(x)], [xin], lambda d: got.append(d) or [None])
            out = layer.conformer_block(xin, dev(lens, np.int32), H, FF, K, scope='blk')
            dout = rng.standard_normal(tuple(out.shape)).astype(np.float32)
            root = torch.zeros(1, device='cuda')
            record([out], [root], lambda _: [dev(dout)])
        tape.backward(root)
    P = {n: store.vars['blk/' + n].data.cpu().numpy() for n in R.NAMES}
    ref, dh, G = R.block(x, lens, P, H, dout)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=2e-4 * np.abs(ref).max())
    np.testing.assert_allclose(got[0].cpu().numpy(), dh, rtol=0, atol=2e-4 * np.abs(dh).max())
    for n in R.NAMES:
        np.testing.assert_allclose(store.vars['blk/' + n].grad.cpu().numpy(), G[n], rtol=0, atol=2e-4 * np.abs(G[n]).max(), err_msg=n)


@pytest.mark.parametrize('conv', [False, True])
def test_the_encoder_through_the_recipe_api(conv):
    """encoder = conformer from cfg text, with and without conv_channels: a finite CTC loss, the same loss bits from the
    same seed, the encoded lengths (the inputs', or the pooled ones) and zeros past each length"""
    over = dict({'encoder.encoder': 'conformer', 'encoder.conv_kernel': 7},
                **({'encoder.conv_channels': '32 32', 'encoder.feature_blocks': 3} if conv else {}))
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)
    raw, losses = data.batch(0), []
    lens = raw['input_seq_length']['features']
    for _ in range(2):
        ops.set_seed(0)
        tr = make_trainer(data, **over)
        b = tr.to_device(raw)
        losses.append(tr.step(b).cpu().numpy().reshape(-1)[0])
        with vs.as_default(tr.model.store):
            enc, enc_lens = tr.model.encoder(b['inputs'], b['input_seq_length'], False)
        got = np.asarray(getattr(enc_lens['features'], 'host', enc_lens['features']))
        assert list(got) == list(-(-(-(-lens // 2)) // 2) if conv else lens)
        e = enc['features'].cpu().numpy()
        assert np.all(np.isfinite(e)) and all(np.all(e[i, L:] == 0) for i, L in enumerate(got))
    assert np.isfinite(losses[0]) and losses[0].view(np.int32) == losses[1].view(np.int32)
