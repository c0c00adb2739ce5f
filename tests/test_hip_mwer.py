"""The MWER kernels (nabu_amd/csrc/mwer.hip) against their float64 restatement (tests/mwer_ref.py), and the MWER step
end to end on the tiny Speller of tests/beam_joint_cases.py (tests/mwer_cases.py).

The bars of the loss kernel are norm-wise relative errors: the larger of the bar xent_kernel is held to
(tests/test_hip_xent_smooth.py: loss 1e-6, dlogits 1e-5) and 4 x the error of the float32 restatement of
tests/mwer_ref.py on the same inputs, measured on the CPU and written down in F32_ERR below (the 4 covers another
summation order).  With the logits of these cases the posterior is close to one-hot, so the float32 error stays near
1e-7 and the xent_kernel bars decide everywhere."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip
from nabu_amd import ops
from tests import mwer_cases as MC
from tests import mwer_ref as ref
from tests.test_mwer_ref import hand_written_beams

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -12345.5
PAD = 64
XENT_LOSS_BAR, XENT_GRAD_BAR = 1e-6, 1e-5

# case -> (loss, dlogits): norm-wise relative error of mwer_ref.loss_grad(dtype=float32) against float64, on the CPU
F32_ERR = {
    'N1-L1-C2-all': (2.93e-08, 6.44e-08), 'N1-L1-C41-one': (4.30e-08, 6.05e-08), 'N1-L1-C1023-slot0': (2.49e-08, 5.10e-08),
    'N1-L19-C2-one': (4.29e-08, 9.27e-08), 'N1-L19-C41-slot0': (3.87e-08, 7.52e-08), 'N1-L19-C1023-all': (4.06e-08, 5.63e-08),
    'N1-L300-C2-slot0': (3.07e-08, 8.51e-08), 'N1-L300-C41-all': (3.80e-08, 7.69e-08),
    'N1-L300-C1023-one': (3.38e-08, 5.91e-08), 'N2-L1-C2-one': (1.36e-08, 8.05e-08), 'N2-L1-C41-slot0': (1.76e-08, 6.14e-08),
    'N2-L1-C1023-all': (7.18e-08, 1.12e-07), 'N2-L19-C2-slot0': (2.35e-08, 7.52e-08), 'N2-L19-C41-all': (6.04e-08, 1.02e-06),
    'N2-L19-C1023-one': (6.39e-08, 6.05e-08), 'N2-L300-C2-all': (2.08e-08, 8.29e-08), 'N2-L300-C41-one': (5.76e-08, 7.86e-08),
    'N2-L300-C1023-slot0': (3.16e-08, 5.64e-08), 'N4-L1-C2-slot0': (3.69e-08, 6.01e-08), 'N4-L1-C41-all': (2.81e-08, 1.66e-07),
    'N4-L1-C1023-one': (3.04e-08, 3.44e-08), 'N4-L19-C2-all': (6.67e-08, 7.78e-08), 'N4-L19-C41-one': (1.55e-08, 8.93e-08),
    'N4-L19-C1023-slot0': (3.47e-08, 5.63e-08), 'N4-L300-C2-one': (6.84e-08, 8.75e-08), 'N4-L300-C41-slot0': (4.53e-08, 8.01e-08),
    'N4-L300-C1023-all': (2.39e-08, 5.95e-08), 'N16-L1-C2-all': (6.18e-08, 1.24e-07), 'N16-L1-C41-one': (2.97e-08, 5.43e-08),
    'N16-L1-C1023-slot0': (4.09e-08, 4.73e-08), 'N16-L19-C2-one': (2.88e-08, 7.91e-08), 'N16-L19-C41-slot0': (3.91e-08, 7.69e-08),
    'N16-L19-C1023-all': (4.74e-08, 5.83e-08), 'N16-L300-C2-slot0': (6.74e-08, 8.79e-08), 'N16-L300-C41-all': (2.30e-08, 7.24e-08),
    'N16-L300-C1023-one': (4.80e-08, 6.07e-08), 'N16-L500-C2-all': (6.02e-08, 8.31e-08),
}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    return x.detach().cpu().numpy()


def framed(numel, phase=0, dtype=torch.float32):
    """a sentinel-filled buffer and the view of `numel` words inside it, `phase` words off a 16-byte boundary"""
    buf = torch.full((numel + 2 * PAD + 4,), SENTINEL, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + phase:PAD + phase + numel]


def untouched(buf, numel, phase=0):
    b = host(buf)
    s = b.dtype.type(SENTINEL)
    return bool(np.all(b[:PAD + phase] == s) and np.all(b[PAD + phase + numel:] == s))


def raw_loss(logits, stk_targets, stk_len, errs, valid, ce_weight, scale, phase=0):
    """the entry point itself, every output inside a sentinel-filled buffer: (loss, risk, nll_ref, dlogits, clean)"""
    rows, L, C = logits.shape
    NB = valid.numel()
    B = rows - NB
    small = [framed(B) for _ in range(3)]
    dbuf, dl = framed(rows * L * C, phase)
    _hip.check(_hip.lib().nabu_mwer_loss_grad(B, NB // B, L, C, stk_targets.shape[1], _hip.ptr(logits), _hip.ptr(stk_targets),
                                              _hip.ptr(stk_len), _hip.ptr(errs), _hip.ptr(valid), ce_weight, scale,
                                              *[_hip.ptr(v) for _, v in small], _hip.ptr(dl), _hip.stream()),
               'nabu_mwer_loss_grad')
    clean = all(untouched(b, B) for b, _ in small) and untouched(dbuf, rows * L * C, phase)
    return [host(v).copy() for _, v in small] + [host(dl).reshape(rows, L, C).copy(), clean]


@pytest.mark.parametrize('case', ref.loss_cases(), ids=ref.case_id)
def test_loss_kernel_against_float64(case):
    N, L, C, _ = case
    B = ref.LOSS_B
    inputs = ref.loss_inputs(case)
    logits, stk_targets, stk_len, errs, valid = inputs
    assert stk_len.min() == 1 and stk_len.max() == L
    scale = 1.0 / B
    want = ref.loss_grad(*inputs, ref.LOSS_CE_WEIGHT, scale)
    d_in = [dev(a) for a in inputs]
    loss, risk, nll_ref, d, clean = raw_loss(*d_in, ref.LOSS_CE_WEIGHT, scale)
    assert clean
    f32_loss, f32_grad = F32_ERR[ref.case_id(case)]
    loss_bar, grad_bar = max(XENT_LOSS_BAR, 4 * f32_loss), max(XENT_GRAD_BAR, 4 * f32_grad)
    errors = [ref.rel_err(loss, want[0]), ref.rel_err(risk, want[1]), ref.rel_err(nll_ref, want[2]), ref.rel_err(d, want[3])]
    print('%s: loss %.3g (bar %.3g)  risk %.3g  nll_ref %.3g  dlogits %.3g (bar %.3g)'
          % (ref.case_id(case), errors[0], loss_bar, errors[1], errors[2], errors[3], grad_bar))
    assert errors[0] <= loss_bar and errors[1] <= loss_bar and errors[2] <= loss_bar
    assert errors[3] <= grad_bar
    # the exact zeros: past stk_len, and on every row of an invalid hypothesis
    rows = (N + 1) * B
    past = np.arange(L)[None, :] >= stk_len[:, None]
    assert not d[past].any()
    assert not d[:N * B][valid == 0].any()
    assert d[N * B:].any() and np.isfinite(d).all()
    # a second call gives the same bits, and so does one whose dlogits sit off the 16-byte phase
    again = raw_loss(*d_in, ref.LOSS_CE_WEIGHT, scale)
    off = raw_loss(*d_in, ref.LOSS_CE_WEIGHT, scale, phase=1)
    assert again[4] and off[4]
    for a, b_, c_ in zip((loss, risk, nll_ref, d), again, off):
        assert np.array_equal(a, b_) and np.array_equal(a, c_)
    assert rows * L * C == d.size


@pytest.mark.parametrize('N', [1, 4])
def test_loss_kernel_exact_zeros(N):
    B, L, C = ref.LOSS_B, 19, 41
    logits, stk_targets, stk_len, errs, valid = ref.loss_inputs((N, L, C, 'all'))
    valid = valid.copy()
    if N > 1:
        valid[1 * B + 2] = 0                                     # one invalid slot whose count differs
    errs = np.full_like(errs, 3)
    if N > 1:
        errs[1 * B + 2] = 9
    d_in = [dev(a) for a in (logits, stk_targets, stk_len, errs, valid)]
    # equal error counts over the valid slots: no hypothesis row moves; N = 1 is the cross-entropy term alone
    loss, risk, nll_ref, d, clean = raw_loss(*d_in, 1.0, 0.2)
    assert clean and not d[:N * B].any() and d[N * B:].any()
    want = ref.loss_grad(logits, stk_targets, stk_len, errs, valid, 1.0, 0.2)
    assert ref.rel_err(d, want[3]) <= XENT_GRAD_BAR
    # (3 times a posterior that sums to 1 only up to its roundings; one hypothesis has p = 1 exactly)
    assert ref.rel_err(risk, np.full(B, 3.0)) <= XENT_LOSS_BAR
    assert N > 1 or (risk == 3).all()
    # ce_weight == 0: the reference rows stay zero, and the loss is the risk
    errs2 = ref.loss_inputs((N, L, C, 'all'))[3]
    loss, risk, nll_ref, d, clean = raw_loss(d_in[0], d_in[1], d_in[2], dev(errs2), d_in[4], 0.0, 0.2)
    assert clean and not d[N * B:].any()
    assert np.array_equal(loss, risk) and np.isfinite(nll_ref).all() and (nll_ref > 0).all()
    assert d[:N * B].any() == (N > 1)
    # no valid slot at all: a risk of 0 and no gradient on the hypothesis rows
    loss, risk, nll_ref, d, clean = raw_loss(d_in[0], d_in[1], d_in[2], dev(errs2), dev(np.zeros_like(valid)), 0.5, 0.2)
    assert clean and not d[:N * B].any() and not risk.any() and d[N * B:].any()


def test_loss_kernel_argument_errors():
    lib = _hip.lib()
    B, L = 2, 3

    def call(N, C, ce=0.5, scale=1.0, null=False, ldt=None):
        rows = (N + 1) * B
        logits = torch.zeros((rows, L, max(C, 1)), device=DEV)
        tg = torch.zeros((rows, L), dtype=torch.int32, device=DEV)
        ln = torch.ones(rows, dtype=torch.int32, device=DEV)
        e = torch.zeros(max(N, 1) * B, dtype=torch.int32, device=DEV)
        out = [torch.zeros(B, device=DEV) for _ in range(3)]
        return lib.nabu_mwer_loss_grad(B, N, L, C, L if ldt is None else ldt, _hip.ptr(logits), _hip.ptr(tg), _hip.ptr(ln),
                                       _hip.ptr(e), _hip.ptr(e), ce, scale, *[_hip.ptr(o) for o in out],
                                       None if null else _hip.ptr(torch.empty_like(logits)), _hip.stream())
    assert call(4, 5) == 0
    for N, C in ((17, 5), (4, 1), (4, 1024)):
        assert call(N, C) == ops.NABU_EUNSUP
        assert lib.nabu_last_error()
    assert b'at most 16' in (call(17, 5), lib.nabu_last_error())[1]
    for kw in (dict(N=0, C=5), dict(N=4, C=0), dict(N=4, C=5, ce=-1.0), dict(N=4, C=5, ce=float('nan')),
               dict(N=4, C=5, ce=float('inf')), dict(N=4, C=5, scale=float('inf')), dict(N=4, C=5, null=True),
               dict(N=4, C=5, ldt=L - 1)):
        assert call(**kw) == -1, kw
    with pytest.raises(_hip.NabuHipError, match='at most 16'):
        ops.mwer_prepare(torch.zeros((1, 17, 2), dtype=torch.int32, device=DEV), torch.zeros((1, 17), dtype=torch.int32, device=DEV),
                         torch.zeros((1, 17), device=DEV), torch.zeros((1, 2), dtype=torch.int32, device=DEV),
                         torch.ones(1, dtype=torch.int32, device=DEV), 5)


# ---------------------------------------------------------------------------------------------------- prepare and tile
def check_prepare(seq, lengths, scores, targets, target_len, C, ldt=None, view=False):
    want = ref.prepare(seq, lengths, scores, targets, target_len, C, ldt)
    seq_d = dev(seq)
    if view:                          # the beam search's buffer cut to the steps it took: a longer row stride
        B, N, S = seq.shape
        full = torch.full((B, N, S + 3), -7, dtype=torch.int32, device=DEV)
        full[:, :, :S] = seq_d
        seq_d = full[:, :, :S]
    got = ops.mwer_prepare(seq_d, dev(lengths), dev(scores), dev(targets), dev(target_len), C, ldt)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32
        np.testing.assert_array_equal(host(g), w)
    errs = ops.edit_distance(got[0][:len(want[2])], got[2], dev(np.tile(targets, (seq.shape[1], 1))),
                             dev(np.tile(np.maximum(target_len - 1, 0), seq.shape[1])))
    np.testing.assert_array_equal(host(errs), ref.errors(want[0], want[2], targets, target_len))
    return want


@pytest.mark.parametrize('view', [False, True])
def test_prepare_on_hand_written_beams(view):
    _, _, _, valid = check_prepare(*hand_written_beams(), 7, view=view)
    np.testing.assert_array_equal(valid.reshape(4, 2), [[1, 1], [0, 1], [1, 0], [0, 1]])
    check_prepare(*hand_written_beams(), 7, ldt=9, view=view)
    seq = np.array([[[1, 2], [1, 2]]], np.int32)                     # a duplicate of a spare slot stays valid
    check_prepare(seq, np.array([[2, 2]], np.int32), np.array([[-ref.FLT_MAX, -1.0]], np.float32),
                  np.array([[1, 6]], np.int32), np.array([2], np.int32), 7)


@pytest.mark.parametrize('seed', range(4))
def test_prepare_on_random_beams(seed):
    B, N, S, C = 3, 4, 6, 4
    rng = np.random.RandomState(seed)
    seq = rng.randint(0, C - 1, size=(B, N, S)).astype(np.int32)
    lengths = rng.randint(0, S + 1, size=(B, N)).astype(np.int32)
    seq[0, 2], lengths[0, 2] = seq[0, 0], lengths[0, 0]              # a duplicate, and a pair that differs past the length
    seq[1, 3, :lengths[1, 1]], lengths[1, 3] = seq[1, 1, :lengths[1, 1]], lengths[1, 1]
    lengths[2, 1] = S + 2                                            # clamped to S
    scores = (-rng.uniform(0, 9, size=(B, N))).astype(np.float32)
    scores[rng.uniform(size=(B, N)) < 0.2] = -ref.FLT_MAX
    target_len = rng.randint(1, 9, size=B).astype(np.int32)
    targets = rng.randint(0, C - 1, size=(B, 8)).astype(np.int32)
    for b in range(B):
        targets[b, target_len[b] - 1] = C - 1
    _, _, _, valid = check_prepare(seq, lengths, scores, targets, target_len, C, view=bool(seed % 2))
    assert valid.reshape(N, B)[2, 0] == 0 or scores[0, 0] < -1e30 or scores[0, 2] < -1e30


@pytest.mark.parametrize('R', [1, 5, 17])
@pytest.mark.parametrize('F', [1, 3, 4, 1028])
def test_tile_rows_forward_and_backward(F, R):
    """forward: exact.  backward: R float32 terms added in the order r = 0..R-1, so |error| <= (R - 1) 2^-24 sum_r |dy_r|
    per element against the float64 sum (every partial sum is at most that sum in magnitude)."""
    B = 3
    rng = np.random.RandomState(100 * F + R)
    x = rng.standard_normal((B, F)).astype(np.float32)
    dy = rng.standard_normal((R * B, F)).astype(np.float32)
    want_dx = ref.tile_bwd(dy, R)
    bound = (R - 1) * 2.0 ** -24 * np.abs(dy.astype(np.float64)).reshape(R, B, F).sum(0)
    lib = _hip.lib()
    for phase_one, phase_many in ((0, 0), (1, 0), (0, 1), (3, 2)):          # 16-byte phases of x / dx and of y / dy
        xbuf, xv = framed(B * F, phase_one)
        xv.copy_(dev(x).reshape(-1))
        ybuf, yv = framed(R * B * F, phase_many)
        _hip.check(lib.nabu_rows_tile_f32(R, B, F, _hip.ptr(xv), _hip.ptr(yv), _hip.stream()), 'nabu_rows_tile_f32')
        assert untouched(ybuf, R * B * F, phase_many)
        np.testing.assert_array_equal(host(yv).reshape(R * B, F), ref.tile(x, R))
        dybuf, dyv = framed(R * B * F, phase_many)
        dyv.copy_(dev(dy).reshape(-1))
        outs = []
        for _ in range(2):
            dxbuf, dxv = framed(B * F, phase_one)
            _hip.check(lib.nabu_rows_tile_bwd_f32(R, B, F, _hip.ptr(dyv), _hip.ptr(dxv), _hip.stream()),
                       'nabu_rows_tile_bwd_f32')
            assert untouched(dxbuf, B * F, phase_one)
            outs.append(host(dxv).reshape(B, F).copy())
        assert np.array_equal(outs[0], outs[1])
        assert np.all(np.abs(outs[0].astype(np.float64) - want_dx) <= bound)
        if R == 1:
            np.testing.assert_array_equal(outs[0], dy)
    assert lib.nabu_rows_tile_f32(0, B, F, _hip.ptr(xv), _hip.ptr(yv), _hip.stream()) == -1
    assert lib.nabu_rows_tile_bwd_f32(R, B, F, None, _hip.ptr(xv), _hip.stream()) == -1


def test_tile_rows_is_a_tape_node():
    from nabu_amd.autodiff import Tape, record
    from nabu_amd.neuralnetworks.components import ops as nops
    x = torch.randn((3, 5, 7), device=DEV)
    src = x.clone()
    got = []
    with Tape() as tape:
        record([src], [x], lambda g: got.append(g) or [None])
        y = nops.tile_rows(x, 4)
        root = torch.zeros(1, device=DEV)
        dy = torch.randn_like(y)
        record([y], [root], lambda g: [dy])
    assert y.shape == (12, 5, 7) and torch.equal(y, x.repeat(4, 1, 1))
    tape.backward(root)
    torch.testing.assert_close(got[0], dy.view(4, 3, 5, 7).sum(0), rtol=1e-6, atol=1e-6)
    with Tape():                                         # a leaf (raw features) needs no gradient node
        assert nops.tile_rows(src, 2).shape == (6, 5, 7) and not Tape.current.ops


# ------------------------------------------------------------------------------------------------------ end to end
def tiny_speller(kind):
    """the decoder, its store holding the case's parameters, the encoded inputs and their lengths on the device"""
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import SeqLen
    from tests import beam_joint_cases as J
    from tests.test_hip_beam_joint import device_state
    from tests.test_hip_multi_speller import NAMES, make_decoder
    attention, p, encs, enc_lens, targets, target_len = MC.case(kind)
    c = J.SEARCH
    dec = make_decoder(attention, 'softmax', 1, c['U'], J.K_LOC, J.F_LOC, c['C'], extra={'decoder.dropout': 1.0})
    store = vs.VariableStore(seed=0)
    state = device_state(attention, p)
    store.restore_from(state)
    enc_d = {NAMES[m]: dev(e) for m, e in enumerate(encs)}
    lens = {NAMES[m]: SeqLen(l, torch.device(DEV)) for m, l in enumerate(enc_lens)}
    return dec, store, state, enc_d, lens, targets, target_len


@pytest.mark.parametrize('kind', MC.KINDS)
def test_device_nbest_is_the_float64_nbest(kind):
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.trainers import mwer
    from tests import beam_joint_cases as J
    dec, store, state, enc_d, lens, targets, target_len = tiny_speller(kind)
    want, gap, T = MC.brute_force(kind)
    assert gap >= J.MARGIN
    B, N, C = J.SEARCH['B'], MC.N, J.SEARCH['C']
    with vs.as_default(store), vs.variable_scope(dec.scope):
        stk_targets, stk_len, hyp_len, valid, errors, bound = mwer.nbest_targets(
            dec, enc_d, lens, dev(targets), target_len, N, J.SEARCH['S'])
    assert not store.restore and sorted(store.state_dict()) == sorted(state)
    assert bound == max(T + 1, int(target_len.max()))
    stk_targets, stk_len, hyp_len, valid, errors = (host(x) for x in (stk_targets, stk_len, hyp_len, valid, errors))
    for b in range(B):
        seen = set()
        for n in range(N):
            labels, length, _ = want[b][n]
            row = n * B + b
            first = labels not in seen
            seen.add(labels)
            assert valid[row] == int(first)
            expect = list(labels) if first else []
            assert length == len(labels) and hyp_len[row] == len(expect)
            assert list(stk_targets[row, :stk_len[row]]) == expect + [C - 1]
            assert errors[row] == ref.levenshtein(expect, targets[b, :target_len[b] - 1])
        assert list(stk_targets[N * B + b, :stk_len[N * B + b]]) == list(targets[b, :target_len[b]])


class TinyModel(object):
    """what trainers/mwer.py asks of a model: a store, a decoder, and an encoder whose outputs are tape nodes"""

    def __init__(self, dec, store, enc_d, lens):
        self.decoder, self.store, self.enc_d, self.lens = dec, store, enc_d, lens
        self.sources = {k: v.clone() for k, v in enc_d.items()}
        self.got = {}

    def encoder(self, inputs, input_seq_length, is_training):
        from nabu_amd.autodiff import record
        assert is_training
        for k in self.enc_d:
            record([self.sources[k]], [self.enc_d[k]], lambda g, k=k: self.got.__setitem__(k, g) or [None])
        return self.enc_d, self.lens


@pytest.mark.parametrize('kind', MC.KINDS)
def test_mwer_pass_matches_the_float64_chain(kind):
    """the loss, d encoded and every decoder parameter gradient of trainers/mwer.py's pass on the device's own
    hypotheses, against tile -> multi_speller_fwd -> the reference loss -> multi_speller_bwd -> the sum over the slots.
    Bars: those of tests/test_hip_multi_speller.py's check_multi for the same quantities (loss 1e-5 relative, gradients
    2e-4 of the largest entry)."""
    from nabu_amd.autodiff import Tape, SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    from nabu_amd.neuralnetworks.trainers import mwer
    from tests import beam_joint_cases as J
    from tests.test_hip_multi_speller import NAMES, PRE, mech_names
    dec, store, state, enc_d, lens, targets, target_len = tiny_speller(kind)
    model = TinyModel(dec, store, enc_d, lens)
    batch = dict(inputs={}, input_seq_length={}, targets={'text': dev(targets)},
                 target_seq_length={'text': SeqLen(target_len, torch.device(DEV))})
    with Tape() as tape:
        loss, stats = mwer.forward_loss(model, batch, MC.N, J.SEARCH['S'], MC.CE_WEIGHT)
    assert rnn_decoder.dynamic_decode.last[0].sample_prob == 0.0 and rnn_decoder.dynamic_decode.last[0].B == 15
    tape.backward(loss)
    torch.cuda.synchronize()
    data = {k: host(stats[k]) for k in ('stk_targets', 'stk_len', 'errors', 'valid')}
    assert data['valid'].sum() >= 2 * J.SEARCH['B']                     # a list, not a single hypothesis
    rloss, rdencs, rg = MC.float64_chain(kind, data['stk_targets'], data['stk_len'], data['errors'], data['valid'])
    got_loss = float(loss.item())
    print('%s: loss %.6f (float64 %.6f)' % (kind, got_loss, rloss))
    assert abs(got_loss - rloss) / rloss < 1e-5
    rel = lambda a, b_: np.abs(a - b_).max() / (np.abs(b_).max() + 1e-12)
    attention, M = J.SEARCH_KINDS[kind]
    grad = lambda name: host(store.vars[name].grad).astype(np.float64)
    worst = 0.0
    for m in range(M):
        e = rel(host(model.got[NAMES[m]]), rdencs[m])
        worst = max(worst, e)
        assert e < 2e-4, m
        for k, name in mech_names(attention, m).items():
            e = rel(grad(name).reshape(rg['mem'][m][k].shape), rg['mem'][m][k])
            worst = max(worst, e)
            assert e < 2e-4, (m, k)
    for k in ('out_kernel', 'out_bias'):
        assert rel(grad(PRE + 'dense/' + k[4:]), rg[k]) < 2e-4, k
    q = PRE + 'attention_wrapper/multi_rnn_cell/cell_0/lstm_cell/'
    assert rel(grad(q + 'kernel'), rg['lstm'][0]['kernel']) < 2e-4
    assert rel(grad(q + 'bias'), rg['lstm'][0]['bias']) < 2e-4
    print('%s: largest relative gradient error %.3g' % (kind, worst))
    stats_host = mwer.read_stats(stats)
    assert stats_host[0] >= 0 and stats_host[1] > 0 and 0 < stats_host[2] <= 1


def small_trainer(**over):
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    keys = {'encoder.num_units': 32, 'decoder.num_units': 32}
    keys.update(over)
    mc, tc, ec = recipes.load_recipe('cfg3_las_vanilla', **keys)
    data = SyntheticData(4, 64, 40, min_frames=40, min_labels=2, max_labels=6, eos=True, time_reduction=8, seed=78)
    nops.set_seed(11)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=None, expdir=None,
                                               server=None, task_index=0)


def run_steps(tr, n):
    losses = []
    for _ in range(n):
        loss = tr.step(tr.to_device(tr.data.batch(tr.global_step)))
        tr.global_step += 1
        losses.append(host(loss).copy())
    return losses


def test_trainer_switches_to_mwer_at_the_start_step():
    plain = small_trainer()
    plain._create_graph()
    plain_losses = run_steps(plain, 2)
    with pytest.raises(Exception, match='first MWER step'):
        plain.mwer_stats()
    tr = small_trainer(**{'trainer.mwer_nbest': 2, 'trainer.mwer_max_steps': 8, 'trainer.mwer_start_step': 2})
    tr._create_graph()
    losses = run_steps(tr, 2)
    for a, b_ in zip(losses, plain_losses):                  # before the start step: the plain step, bit for bit
        assert a.tobytes() == b_.tobytes()
    assert tr._mwer_stats is None
    before = tr.flat.clone()
    losses += run_steps(tr, 2)
    assert all(np.isfinite(l).all() for l in losses)
    risk, nll_ref, share = tr.mwer_stats()
    print('expected errors %.4f, reference nll %.4f, valid share %.3f' % (risk, nll_ref, share))
    assert risk >= 0 and np.isfinite(nll_ref) and 0 < share <= 1
    assert not torch.equal(tr.flat, before) and bool(torch.isfinite(tr.flat).all())
