"""GPU: conv2d.hip against the float64 restatement (tests/conv_ref.py) at the smallest shapes that reach every branch: odd
K (Cin 1, 3), several channel chunks (Cin 96), every wave arrangement and width (F 1, 5: 1 x 1 / 1 x 2; 21: 2 x 1 / 2 x 2; 41: 4 x 1;
Cout 128: the 128-wide kernel), two uneven column tiles (F 45), times around the tile, lengths 0 .. T."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip, ops as hip, recipes
from nabu_amd.autodiff import Tape, record
from nabu_amd import variables as vs
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.processing.synthetic import SyntheticData
from tests import conv_ref as R

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.5, 64


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def guarded_conv(x, mask, lens, w, bias, plain):
    """nabu_conv3x3_relu_fwd into a sentinel-filled buffer with guard words on both sides: (y, guards untouched)"""
    B, T, F, Cin = x.shape
    Cout = w.shape[3]
    n = B * T * F * Cout
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device='cuda')
    args = [dev(x), None if mask is None else dev(mask), dev(lens, np.int32), dev(w), dev(bias)]
    _hip.check(_hip.lib().nabu_conv3x3_relu_fwd(B, T, F, Cin, Cout, _hip.ptr(args[0]), _hip.ptr(args[1]), _hip.ptr(args[2]),
                                                _hip.ptr(args[3]), _hip.ptr(args[4]), int(plain),
                                                buf.data_ptr() + 4 * GUARD, _hip.stream()), 'conv')
    out = buf.cpu().numpy()
    return out[GUARD:GUARD + n].reshape(B, T, F, Cout), bool(np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n:] == SENTINEL))


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('F', [1, 5, 21, 41, 45])
@pytest.mark.parametrize('Cout', [32, 64, 128])
@pytest.mark.parametrize('Cin', [1, 3, 32, 96])
def test_forward_matches_float64_within_the_chain_bound(Cin, Cout, F, masked):
    """|y - ref| <= gamma(9 Cin + 3) (|x| * |w| + |bias|) componentwise: a k-ordered fmaf chain of 9 Cin terms, the bias
    add, and the roundings of the stored operands' products; every word past a length is +0.0, nothing outside is written"""
    tile = hip.conv_tile_t()
    rng = np.random.default_rng(Cin * 1000 + Cout * 10 + F)
    for T in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
        lens = np.clip(np.array([T, 0, 1, tile, T - 1]), 0, T).astype(np.int32)
        x = rng.standard_normal((5, T, F, Cin)).astype(np.float32)
        w, bias = rng.standard_normal((3, 3, Cin, Cout)).astype(np.float32), rng.standard_normal(Cout).astype(np.float32)
        mask = rng.standard_normal(x.shape).astype(np.float32) if masked else None
        y, clean = guarded_conv(x, mask, lens, w, bias, plain=masked)
        xe = x.astype(np.float64) * (mask > 0) if masked else x.astype(np.float64)
        ref = R.conv(xe, lens, w.astype(np.float64), None if masked else bias.astype(np.float64), relu=not masked)
        bound = R.gamma(9 * Cin + 3) * R.conv(np.abs(xe), lens, np.abs(w), None if masked else np.abs(bias), relu=False)
        assert clean and np.all(np.abs(y - ref) <= bound), (T, clean, float(np.max(np.abs(y - ref) - bound)))
        assert all(np.all(y[b, L:].view(np.int32) == 0) for b, L in enumerate(lens)), T


@pytest.mark.parametrize('Cin,Cout,F', [(3, 32, 5), (32, 64, 41), (32, 128, 21)])
def test_an_utterance_does_not_see_its_padding(Cin, Cout, F):
    """alone at T = len, or inside a longer batch whose padding frames hold 1e30: the same bits"""
    tile = hip.conv_tile_t()
    rng = np.random.default_rng(3)
    L, T = tile + 1, 2 * tile + 2
    x = np.full((2, T, F, Cin), 1e30, np.float32)
    x[0, :L] = rng.standard_normal((L, F, Cin))
    w, bias = rng.standard_normal((3, 3, Cin, Cout)).astype(np.float32), rng.standard_normal(Cout).astype(np.float32)
    inside = hip.conv3x3_relu(dev(x), dev([L, T], np.int32), dev(w), dev(bias)).cpu().numpy()
    alone = hip.conv3x3_relu(dev(x[:1, :L]), dev([L], np.int32), dev(w), dev(bias)).cpu().numpy()
    np.testing.assert_array_equal(inside[0, :L].view(np.int32), alone[0].view(np.int32))
    assert np.all(inside[0, L:] == 0)


@pytest.mark.parametrize('B,T', [(2, 5), (5, 9)])                # 4 (b, time tile) pairs: one split; 15: several
@pytest.mark.parametrize('Cin,Cout,F', [(3, 64, 41), (96, 64, 5), (64, 32, 5), (32, 128, 1), (32, 64, 45)])
def test_weight_and_bias_gradient(Cin, Cout, F, B, T):
    """|dw - ref| <= gamma(R + S + 3) (|x| * |g|): a reduction over at most R = B T F positions in S partial sums;
    two calls give the same bits"""
    rng = np.random.default_rng(Cin + Cout + F + B)
    lens = np.clip(np.array([T, 0, 1, 3, T - 1])[:B], 0, T).astype(np.int32)
    x, dy, y = (rng.standard_normal((B, T, F, c)).astype(np.float32) for c in (Cin, Cout, Cout))
    S = _hip.lib().nabu_conv_ws_bytes(B, T, F, Cin, Cout) // ((9 * Cin * Cout + Cout) * 4)
    assert (S == 1) == (B == 2)
    got = []
    for _ in range(2):
        dw, db = torch.full((3, 3, Cin, Cout), SENTINEL, device='cuda'), torch.full((Cout,), SENTINEL, device='cuda')
        hip.conv3x3_bwd_weights(dev(x), dev(dy), dev(y), dev(lens, np.int32), dw, db)
        got.append((dw.cpu().numpy(), db.cpu().numpy()))
    g = dy.astype(np.float64) * (y > 0)
    ref, bound = R.wgrad(x.astype(np.float64), lens, g), R.wgrad(np.abs(x).astype(np.float64), lens, np.abs(g))
    for k in range(2):
        assert np.all(np.abs(got[0][k] - ref[k]) <= R.gamma(B * T * F + S + 3) * bound[k])
        np.testing.assert_array_equal(got[0][k].view(np.int32), got[1][k].view(np.int32))


def test_block_gradients_through_the_tape():
    """layer.conv_block under a tape, input taped: dx, dw, dbias against the restatement (an unflipped w' fails).  Tolerance:
    three chained fp32 products of <= 9 * 32 terms, gamma(300) ~ 2e-5 of the absolute sums; 2e-4 of the largest covers them."""
    rng = np.random.default_rng(11)
    B, T, F, C = 3, 7, 5, 32
    lens = np.array([7, 4, 0], np.int32)
    x = rng.standard_normal((B, T, F, C)).astype(np.float32)
    store, got = vs.VariableStore(seed=4), []
    with vs.as_default(store):
        layer.conv_block(dev(x), dev(lens, np.int32), C, C, scope='blk')          # creates the variables
        p = [store.vars['blk/conv%d/%s' % (i, n)] for i in (0, 1) for n in ('kernel', 'bias')]
        for b in (1, 3):
            p[b].data.normal_()                                     # (biases start at zero: make them count)
        with Tape() as tape:
            xin = dev(x)
            record([dev(x)], [xin], lambda d: got.append(d) or [None])
            out, out_lens = layer.conv_block(xin, dev(lens, np.int32), C, C, scope='blk')
            dout = rng.standard_normal(tuple(out.shape)).astype(np.float32)
            root = torch.zeros(1, device='cuda')
            record([out], [root], lambda _: [dev(dout)])
        tape.backward(root)
    params = [[v.data.cpu().numpy().astype(np.float64) for v in p]]
    assert list(out_lens.host) == [4, 2, 0]
    y0 = R.conv(x.astype(np.float64), lens, params[0][0], params[0][1])
    y1 = R.conv(y0, lens, params[0][2], params[0][3])
    grads, dx = R.frontend_bwd(dout.astype(np.float64), [(x.astype(np.float64), lens, y0, y1, params[0][0], params[0][2])])
    for v, g in zip(p, grads[0]):
        np.testing.assert_allclose(v.grad.cpu().numpy(), g, rtol=0, atol=2e-4 * np.abs(g).max())
    np.testing.assert_allclose(got[0].cpu().numpy(), dx, rtol=0, atol=2e-4 * np.abs(dx).max())


@pytest.mark.parametrize('T,F,C', [(5, 5, 3), (4, 6, 32), (1, 1, 1)])
def test_pool_is_exact(T, F, C):
    """bit-equal both ways: odd and even T and F, odd lengths, and a window whose only valid element is negative"""
    rng = np.random.default_rng(T + F)
    lens = np.clip(np.array([T, 3, 1, 0]), 0, T).astype(np.int32)
    x = rng.standard_normal((4, T, F, C)).astype(np.float32)
    x[2, 0] = -np.abs(x[2, 0])                              # len 1: every window of row 2 has valid elements < 0 only
    x[0, :2, :2, 0] = 1.0                                   # a tie: the first element takes the gradient
    y = hip.maxpool2x2(dev(x), dev(lens, np.int32))
    np.testing.assert_array_equal(y.cpu().numpy().view(np.int32), R.pool(x, lens).view(np.int32))
    dy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    dx = hip.maxpool2x2_bwd(dev(x), dev(lens, np.int32), dev(dy)).cpu().numpy()
    np.testing.assert_array_equal(dx.view(np.int32), R.pool_bwd(x, lens, dy).view(np.int32))


def make_trainer(recipe, data, **over):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0)


@pytest.mark.parametrize('enc,recipe,over', [('DBLSTM', 'cfg1_dblstm_ctc', {}),
                                             ('Listener', 'cfg2_listener_ctc', {'encoder.num_layers': 1})])
def test_front_end_through_the_recipe_api(enc, recipe, over, monkeypatch):
    from nabu_amd.neuralnetworks.trainers import loss_functions
    over = dict(over, **{'encoder.num_units': 16, 'trainer.batch_size': 3})
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)
    seen = {}
    inner = layer.conv_frontend

    def spy(*a, **k):
        out, lens = inner(*a, **k)
        tap = out.view_as(out)
        record([out], [tap], lambda d: seen.__setitem__('dout', d) or [d])
        seen.update(out=tap, lens=lens)
        return tap, lens
    monkeypatch.setattr(layer, 'conv_frontend', spy)
    ops.set_seed(0)
    tr = make_trainer(recipe, data, **dict(over, **{'encoder.conv_channels': '32 32', 'encoder.feature_blocks': 3}))
    raw = data.batch(0)
    batch = tr.to_device(raw)
    with Tape() as tape:
        logits, lsl = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'], batch['target_seq_length'], True)
        loss = loss_functions.CTC(batch['targets'], logits, lsl, batch['target_seq_length'])
    tape.backward(loss)
    lens = raw['input_seq_length']['features']
    pre = '%s/features/frontend/block%%d/conv%%d/%%s' % enc
    var = tr.model.store.vars
    names = [[pre % (i, j, n) for j in (0, 1) for n in ('kernel', 'bias')] for i in (0, 1)]
    params = [[var[n].data.cpu().numpy().astype(np.float64) for n in blk] for blk in names]
    ref, ref_lens, caches = R.frontend_fwd(raw['inputs']['features'].astype(np.float64), lens, params, 3)
    assert list(seen['lens'].host) == list(seen['lens'].dev.cpu().numpy()) == list(ref_lens) == list(-(-(-(-lens // 2)) // 2))
    np.testing.assert_allclose(seen['out'].cpu().numpy(), ref, rtol=0, atol=2e-4 * np.abs(ref).max())
    grads, _ = R.frontend_bwd(seen['dout'].cpu().numpy().astype(np.float64), caches)
    for blk, gs in zip(names, grads):
        for n, g in zip(blk, gs):
            np.testing.assert_allclose(var[n].grad.cpu().numpy(), g, rtol=0, atol=2e-4 * max(np.abs(g).max(), 1e-30), err_msg=n)
    # without the key: no frontend/ variable, the same random offsets as ever (none: regularisation is off)
    ops.set_seed(0)
    plain = make_trainer(recipe, data, **over)
    plain.step(plain.to_device(raw))
    assert not any('frontend/' in n for n in plain.model.store.order) and ops.global_rng().offset == 0


@pytest.mark.parametrize('key,value', [('conv_channels', '64 x'), ('conv_channels', '48'), ('conv_channels', '0'),
                                       ('conv_channels', '32 32 32 32'), ('conv_channels', ''), ('feature_blocks', '2')])
def test_refusals(key, value):
    data = SyntheticData(2, 12, 15, min_frames=8, min_labels=1, max_labels=1, time_reduction=4, seed=7)
    over = {'encoder.num_units': 16, 'trainer.batch_size': 2, 'encoder.conv_channels': '32', 'encoder.' + key: value}
    for recipe in ('cfg1_dblstm_ctc', 'cfg2_listener_ctc'):
        with pytest.raises(ValueError, match=key):
            tr = make_trainer(recipe, data, **over)
            tr.step(tr.to_device(data.batch(0)))          # (feature_blocks is checked where the features are seen)
    from nabu_amd.neuralnetworks.models.ed_encoders import dnn
    with pytest.raises(Exception, match='conv_channels'):
        dnn.DNN(recipes.load_recipe('dnn_hybrid_wsj', **{'encoder.conv_channels': '32'})[0], None)
