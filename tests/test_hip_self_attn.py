"""GPU: self_attn.hip against the float64 restatement (tests/self_attn_ref.py) at the smallest shapes that reach every
branch: one key, sizes around the streamed tile (k = 32) and the owned tile (q = 128), several owned tiles, ~300 frames;
lengths 0 .. T in every batch, a row stride with spare columns, both head widths, one head and three."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip, ops as hip, recipes
from nabu_amd.autodiff import Tape, record
from nabu_amd import variables as vs
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import self_attn_ref as R

pytestmark = pytest.mark.gpu
SENTINEL, GUARD, U = -7.5, 64, 2.0 ** -24
TQ, TK = 128, 32                        # nabu_self_attn_tile_q / _k (asserted below)
TS = [1, TK - 1, TK, TK + 1, TQ + 1, 2 * max(TQ, TK) + 3, 301]
BWD_FACTOR = 8.0                        # see test_backward_...: the next power of two above twice the measured 2.16


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def batch(rng, T, H, dk, regime='normal'):
    """(qkv [5,T,ld] with ld = 3D + 4, lens): q, k ~ N(0,1); all scores of a query equal; scores spread to +-1e4"""
    D = H * dk
    lens = np.clip(np.array([T, 0, 1, TK, T - 1]), 0, T).astype(np.int32)
    qkv = rng.standard_normal((5, T, 3 * D + 4)).astype(np.float32)
    if regime == 'equal':
        qkv[:, :, D:2 * D] = qkv[:, :1, D:2 * D]
    if regime == 'spread':
        qkv[:, :, :2 * D] *= np.float32(np.sqrt(1e4 / 3.0))
    return qkv, lens


def guarded(shape):
    """(buffer, view): a sentinel-filled buffer with GUARD words on either side of the view a kernel writes"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def clean(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def forward(qkv, lens, H, dk):
    """nabu_self_attn_fwd into guarded buffers: (o, lse, guards untouched)"""
    B, T, ld = qkv.shape
    (bo, o), (bl, lse), q_dev, len_dev = guarded((B, T, H * dk)), guarded((B, H, T)), dev(qkv), dev(lens, np.int32)
    _hip.check(_hip.lib().nabu_self_attn_fwd(B, T, H, dk, _hip.ptr(q_dev), ld, _hip.ptr(len_dev), o.data_ptr(),
                                             lse.data_ptr(), _hip.stream()), 'fwd')
    return o.cpu().numpy(), lse.cpu().numpy(), clean(bo) and clean(bl)


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('H', [1, 3])
@pytest.mark.parametrize('dk', [32, 64])
def test_forward_within_the_derived_bound_and_backward_at_the_floor(dk, H, T):
    """|o - ref| <= (expm1(2 E) + gamma(L + c2)) A componentwise, E = gamma(dk + 2) max_j |q|.|k_j| / sqrt(dk),
    A = sum_j p_j |v_j|, L = len, nt = ceil(L / 32), from the kernel's operation order (include/nabu_hip.h):
      * a score is a dk-term fmaf chain times fl(1/sqrt(dk)), dk + 2 roundings: every scaled score is off by at most E, every
        probability by a factor e^(+-E), numerator and denominator of o by that factor each: expm1(2 E);
      * the numerator is an L-term fmaf chain over the keys with one rescale per key tile, the denominator an L-term sum
        with one multiply and one add more per tile, then one division: (L + nt) + (L + 2 nt) + 1 roundings;
      * a probability carries the exponential's error once, and once more per rescale, above and below: 2 (nt + 1) eps.
        eps is NOT derived: it is measured here as the largest error, in units of u A, of the float32 numpy restatement
        of the same formulas on the same inputs (<= 14.8 u for N(0,1) and 3.4 u for equal scores at these shapes; at
        scores of +-1e4 the figure is the restatement's own score rounding, 2e4 u), with a margin of 2;
      so c2 = L + 3 nt + 1 + 2 (nt + 1) (2 eps / u).  lse = m + log(l) is held to expm1(E) + gamma(c2 + 4) (1 + |ref| + E / gamma(dk + 2)).
    Rows >= len are +0.0 bit for bit, the guards untouched, no NaN or inf.  Backward, at four of the T: backward_case."""
    assert hip.self_attn_tiles() == (TQ, TK)
    rng = np.random.default_rng(dk * 1000 + H * 10 + T)
    for regime in ('normal', 'equal', 'spread'):
        qkv, lens = batch(rng, T, H, dk, regime)
        o, lse, ok = forward(qkv, lens, H, dk)
        q3 = qkv[:, :, :3 * H * dk]
        ro, rl, E, A = R.attn_fwd(q3, lens, H, bound=True)
        fo, _ = R.attn_fwd(q3, lens, H, dtype=np.float32)
        eps = float(np.max(np.abs(fo - ro) / np.maximum(A, 1e-300))) / U
        Lr = np.clip(lens, 0, T).astype(np.float64)[:, None, None]
        c2 = Lr + 3 * np.ceil(Lr / TK) + 1 + 2 * (np.ceil(Lr / TK) + 1) * 2 * eps
        Eg = R.gamma(dk + 2) * E                                             # [B,H,T]; repeated over dk: [B,T,D]
        bound = (np.expm1(2 * np.repeat(Eg.transpose(0, 2, 1), dk, axis=2)) + R.gamma(Lr + c2)) * A
        assert ok and np.all(np.isfinite(o)) and np.all(np.isfinite(lse)), (regime, ok)
        assert np.all(np.abs(o - ro) <= bound), regime
        lb = np.expm1(Eg) + R.gamma(c2 + 4) * (1 + np.abs(rl) + E)
        assert np.all(np.abs(lse - rl) <= lb), (regime, float(np.max(np.abs(lse - rl) - lb)))
        for b, L in enumerate(lens):
            assert np.all(o[b, L:].view(np.int32) == 0) and np.all(lse[b, :, L:].view(np.int32) == 0), (regime, b)
    if T in (TK - 1, TK + 1, TQ + 1, 2 * max(TQ, TK) + 3):
        backward_case(rng, dk, H, T)


def backward_case(rng, dk, H, T):
    """dq, dk, dv each: ||got - ref||inf <= BWD_FACTOR ||f32 restatement - ref||inf (both over ||ref||inf: the reference's
    own rounding floor).  Largest ratio measured over all cases: 2.16; the fused order adds one
    rounding per key tile and nothing more, so a ratio above 8 would be a defect.  Rows >= len are +0.0, the spare
    columns of the stride and the guards are untouched, two calls give equal bits."""
    qkv, lens = batch(rng, T, H, dk)
    B, D, ld = 5, H * dk, 3 * H * dk + 4
    do = rng.standard_normal((B, T, D)).astype(np.float32)
    q_dev, len_dev, do_dev = dev(qkv), dev(lens, np.int32), dev(do)
    o, lse = hip.self_attn_fwd(q_dev[:, :, :3 * D], len_dev, H)
    got = []
    for _ in range(2):
        buf, dqkv = guarded((B, T, ld))
        _hip.check(_hip.lib().nabu_self_attn_bwd(B, T, H, dk, _hip.ptr(q_dev), ld, _hip.ptr(o), _hip.ptr(lse), _hip.ptr(do_dev),
                                                 _hip.ptr(len_dev), dqkv.data_ptr(), _hip.stream()), 'bwd')
        got.append(dqkv.cpu().numpy())
        assert clean(buf)
    np.testing.assert_array_equal(got[0].view(np.int32), got[1].view(np.int32))
    assert np.all(got[0][:, :, 3 * D:] == SENTINEL)
    q3 = qkv[:, :, :3 * D]
    ref = R.attn_bwd(q3, *R.attn_fwd(q3, lens, H), do, lens, H)
    f32 = R.attn_bwd(q3, *R.attn_fwd(q3, lens, H, dtype=np.float32), do, lens, H, dtype=np.float32)
    for i, name in enumerate(('dq', 'dk', 'dv')):
        g, r, f = (a[:, :, i * D:(i + 1) * D] for a in (got[0], ref, f32))
        err, floor = np.abs(g - r).max(), np.abs(f - r).max()
        assert err <= BWD_FACTOR * floor, (name, err / floor)
        assert all(np.all(g[b, L:].view(np.int32) == 0) for b, L in enumerate(lens)), name


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
        o, lse = hip.self_attn_fwd(dev(x), dev(lens, np.int32), H)
        dqkv = hip.self_attn_bwd(dev(x), o, lse, dev(d), dev(lens, np.int32), H)
        res.append([t.cpu().numpy() for t in (o, lse.transpose(1, 2), dqkv)])            # all [B, T, .]
    for inside, alone in zip(*res):
        np.testing.assert_array_equal(inside[0, :L].view(np.int32), alone[0].view(np.int32))
        assert np.all(inside[0, L:] == 0)


def test_one_block_through_the_tape():
    """layer.self_attention_block under a tape at gemm_precision f32, input taped: the output, dh and every parameter
    gradient against the float64 block, with the yardstick of test_hip_conv.py's block test (2e-4 of the largest entry)"""
    rng = np.random.default_rng(11)
    B, T, D, H, FF = 3, 9, 64, 2, 128
    lens, x = np.array([9, 4, 0], np.int32), rng.standard_normal((B, T, D)).astype(np.float32)
    store, got, layer.GEMM_PRECISION[0] = vs.VariableStore(seed=4), [], 'f32'
    with vs.as_default(store):
        layer.self_attention_block(dev(x), dev(lens, np.int32), H, FF, scope='blk')       # creates the variables
        for n in R.NAMES:
            if not n.endswith('weights'):
                store.vars['blk/' + n].data.normal_()              # (biases and betas start at zero: make them count)
        with Tape() as tape:
            xin = dev(x)
            record([dev(x)], [xin], lambda d: got.append(d) or [None])
            out = layer.self_attention_block(xin, dev(lens, np.int32), H, FF, scope='blk')
            dout = rng.standard_normal(tuple(out.shape)).astype(np.float32)
            root = torch.zeros(1, device='cuda')
            record([out], [root], lambda _: [dev(dout)])
        tape.backward(root)
    P = {n: store.vars['blk/' + n].data.cpu().numpy().astype(np.float64) for n in R.NAMES}
    ref, cache = R.block_fwd(x.astype(np.float64), lens, P, H)
    G, dh = R.block_bwd(dout.astype(np.float64), cache)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=2e-4 * np.abs(ref).max())
    np.testing.assert_allclose(got[0].cpu().numpy(), dh, rtol=0, atol=2e-4 * np.abs(dh).max())
    for n in R.NAMES:
        np.testing.assert_allclose(store.vars['blk/' + n].grad.cpu().numpy(), G[n], rtol=0, atol=2e-4 * np.abs(G[n]).max(), err_msg=n)


def make_trainer(data, **over):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    over = dict({'encoder.encoder': 'transformer', 'encoder.num_units': 64, 'encoder.num_heads': 2, 'encoder.ff_units': 96,
                 'encoder.num_layers': 2, 'encoder.dropout': 0.9, 'trainer.batch_size': 3}, **over)
    mc, tc, ec = recipes.load_recipe('cfg1_dblstm_ctc', **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0)


@pytest.mark.parametrize('conv', [False, True])
def test_the_encoder_through_the_recipe_api(conv):
    """encoder = transformer from cfg text, with and without conv_channels: a finite CTC loss, the encoded lengths (the
    inputs', or the pooled ones), and the same loss bits from the same seed"""
    over = {'encoder.conv_channels': '32 32', 'encoder.feature_blocks': 3} if conv else {}
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
    for key, value, text in (('num_heads', 3, 'not divisible'), ('num_heads', 4, 'head width'), ('layer_norm', 'True', 'layer_norm'),
                             ('recurrent_precision', 'f32', 'recurrent_precision'), ('conv_channels', '48', 'conv_channels')):
        with pytest.raises(ValueError, match=text):                      # refused at construction
            make_trainer(data, **{'encoder.' + key: value})
