"""Joint CTC/attention training on the GPU: a small Listener + Speller with a CTC head (ctc_head = True) trained with
ctc_weight = 0.3 against the float64 composition of the oracle's pieces — listener_fwd, linear_fwd + ctc_loss on the
head, speller_fwd + average_cross_entropy on the cell, and their backward functions.  The model has the size of the
plain recipe in tests/test_hip_speller.py::test_las_training_trajectory_matches_oracle and is held to its bars: 1e-3
(and 1e-4, what fp32 kernels achieve) relative on every step's loss, 2e-4 relative to the largest entry on gradients."""
import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from nabu_amd.processing.synthetic import SyntheticData
from tests.test_hip_model import make_trainer, encoder_layers
from tests.test_hip_speller import speller_params

pytestmark = pytest.mark.gpu

LAM = 0.3
B, T = 4, 64
OVER = {'encoder.num_units': 64, 'decoder.num_units': 32, 'trainer.batch_size': B, 'encoder.gemm_precision': 'f32',
        'decoder.ctc_head': 'True'}
HEAD_W, HEAD_B = 'Speller/ctc_outlayer/weights', 'Speller/ctc_outlayer/biases'


def data():
    # (at most 3 labels: with a repeat between every pair they still fit into the 5 frames of the shortest utterance)
    return SyntheticData(B, T, 40, min_frames=40, min_labels=2, max_labels=3, eos=True, time_reduction=8, seed=3234)


def trainer(d, **over):
    return make_trainer('cfg3_las_vanilla', d, **dict(OVER, **over))


def initial_state(d, **over):
    """the parameters a trainer of this configuration starts from (float32 arrays by name)"""
    tr = trainer(d, **over)
    b0 = tr.to_device(d.batch(0))
    with torch.no_grad():
        tr.model(b0['inputs'], b0['input_seq_length'], b0['targets'], b0['target_seq_length'], False)
    return tr.model.store.state_dict()


class Ref(object):
    """the float64 model: parameters, and one step's loss and gradients"""

    def __init__(self, st):
        self.layers = encoder_layers(st, 'Listener', 3)
        self.p = speller_params(st, 1, 'vanilla')
        self.W, self.b = st[HEAD_W].astype(np.float64), st[HEAD_B].astype(np.float64)
        self.keys = sorted(k for k in self.p if k != 'lstm')

    def flat(self):
        v = []
        for l in self.layers:
            v += [l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias']]
        return v + [self.p[k] for k in self.keys] + [self.p['lstm'][0]['kernel'], self.p['lstm'][0]['bias'], self.W, self.b]

    def assign(self, new):
        for li, l in enumerate(self.layers):
            l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias'] = new[4 * li:4 * li + 4]
        o = 4 * len(self.layers)
        for i, k in enumerate(self.keys):
            self.p[k] = new[o + i]
        self.p['lstm'][0]['kernel'], self.p['lstm'][0]['bias'], self.W, self.b = new[-4:]

    def step(self, batch, lam=LAM, smoothing=0.0):
        """(joint loss, attention loss, flat gradients in the order of flat())"""
        assert smoothing == 0.0
        y, yl = batch['targets']['text'], batch['target_seq_length']['text']
        enc, el, caches = O.listener_fwd(batch['inputs']['features'].astype(np.float64),
                                         batch['input_seq_length']['features'], self.layers)
        lg, ll, cache = O.speller_fwd(enc, el, y, yl, self.p, 'vanilla')
        att, dlg = O.average_cross_entropy(lg, y, ll, yl)
        denc, g = O.speller_bwd((1 - lam) * dlg, cache)
        head = O.linear_fwd(enc, self.W, self.b)
        nll, dhead = O.ctc_loss(head, el, y, yl - 1)
        dh, dW, db = O.linear_bwd(lam * dhead / len(yl), enc, self.W)
        _, gl = O.listener_bwd(denc + dh, caches)
        grads = []
        for l in gl:
            grads += [l['fw_kernel'], l['fw_bias'], l['bw_kernel'], l['bw_bias']]
        grads += [g[k] for k in self.keys] + [g['lstm'][0]['kernel'], g['lstm'][0]['bias'], dW, db]
        return (1 - lam) * att + lam * nll.mean(), att, grads

    def names(self):
        from tests.test_hip_model import CELL
        from tests.test_hip_speller import grad_names
        n = []
        for l in range(len(self.layers)):
            pre = 'Listener/features/layer%d/%s' % (l, 'BLSTM/' if l < 3 else '')
            n += [pre + CELL % (d, w) for d in ('fw', 'bw') for w in ('kernel', 'bias')]
        m = grad_names(1, 'vanilla')
        q = 'Speller/decoder/attention_wrapper/multi_rnn_cell/cell_0/lstm_cell/'
        return n + [m[k] for k in self.keys] + [q + 'kernel', q + 'bias', HEAD_W, HEAD_B]


def test_the_head_adds_two_variables_under_the_decoder_scope_and_nothing_else():
    d = data()
    with_head, plain = initial_state(d), initial_state(d, **{'decoder.ctc_head': 'False'})
    assert sorted(set(with_head) - set(plain)) == [HEAD_B, HEAD_W] and not set(plain) - set(with_head)
    assert with_head[HEAD_W].shape == (128, 40) and not with_head[HEAD_B].any()
    absent = initial_state(d, **{'decoder.ctc_head': 'False'})
    for k in plain:                       # the variables of a model without the key, and the draws that made them
        np.testing.assert_array_equal(plain[k], absent[k])
        np.testing.assert_array_equal(plain[k], with_head[k])


def test_one_step_loss_and_every_gradient_match_float64():
    from nabu_amd.neuralnetworks.trainers import loss_functions
    d = data()
    tr = trainer(d, **{'trainer.ctc_weight': LAM})
    tr._create_graph()
    ref = Ref(initial_state(d))
    tape, loss = tr._forward_loss(tr.to_device(d.batch(0)))
    tape.backward(loss)
    loss_functions.check_status()
    want, att, grads = ref.step(d.batch(0))
    assert abs(want - att) > 0.05 * abs(att)                  # the CTC term is a visible part of the loss
    assert abs(float(loss.item()) - want) / abs(want) < 1e-5
    got = {v.name: v.grad.cpu().numpy().astype(np.float64) for v in tr.model.variables}
    assert sorted(got) == sorted(ref.names())
    for name, g in zip(ref.names(), grads):
        a = got[name].reshape(g.shape)
        assert np.abs(a - g).max() / (np.abs(g).max() + 1e-12) < 2e-4, name


def test_ten_step_trajectory_matches_float64():
    d = data()
    tr = trainer(d, **{'trainer.ctc_weight': LAM})
    losses = [float(tr.step(tr.to_device(d.batch(s))).item()) for s in range(10)]
    ref = Ref(initial_state(d))
    vals = ref.flat()
    ms, vs_ = [np.zeros_like(v) for v in vals], [np.zeros_like(v) for v in vals]
    want = []
    for s in range(10):
        loss, _, grads = ref.step(d.batch(s))
        want.append(loss)
        new = []
        for i, (v, g) in enumerate(zip(ref.flat(), grads)):
            v2, ms[i], vs_[i] = O.clip_adam_update(v, g, ms[i], vs_[i], s + 1, tr_lr(tr, s))
            new.append(v2)
        ref.assign(new)
    rel = np.abs(np.array(losses) - np.array(want)) / np.abs(want)
    print('largest relative loss error over 10 steps: %.3g' % rel.max())
    assert rel.max() < 1e-3, (losses, want)
    assert rel.max() < 1e-4, (losses, want)


def tr_lr(tr, step):
    """the learning rate of update `step` (exponential decay over the run, trainer.learning_rate)"""
    return (float(tr.conf['initial_learning_rate'])
            * float(tr.conf['learning_rate_decay']) ** (float(step) / tr._graph['num_steps']))


def test_a_head_without_weight_trains_as_the_plain_model_and_gets_no_gradient():
    d = data()
    plain = trainer(d, **{'decoder.ctc_head': 'False'})
    head = trainer(d, **{'trainer.ctc_weight': 0})
    for s in range(2):
        a, b = plain.step(plain.to_device(d.batch(s))), head.step(head.to_device(d.batch(s)))
        assert torch.equal(a, b)
    st = head.model.store.state_dict()
    ref = initial_state(d)
    np.testing.assert_array_equal(st[HEAD_W], ref[HEAD_W])
    np.testing.assert_array_equal(st[HEAD_B], ref[HEAD_B])
    ps = plain.model.store.state_dict()
    for k in ps:
        np.testing.assert_array_equal(ps[k], st[k])


def test_weight_with_label_smoothing_and_two_micro_batches():
    """ctc_weight = 0.3 with label_smoothing = 0.1 (attention term only) and numbatches_to_aggregate = 2: the loss is the
    mean over the two micro-batches of 0.7 * smoothed cross-entropy + 0.3 * CTC, in float64 from the device's logits
    of a forward pass at the same parameters"""
    from tests import xent_smooth_ref as XS
    d = data()
    over = {'trainer.ctc_weight': LAM, 'trainer.label_smoothing': 0.1, 'trainer.numbatches_to_aggregate': 2}
    tr = trainer(d, **over)
    st0 = initial_state(d)
    batches = [d.batch(0), d.batch(1)]
    loss = float(tr.step_accumulated([tr.to_device(b) for b in batches]).item())
    ref = Ref(st0)
    want = []
    for b in batches:
        y, yl = b['targets']['text'], b['target_seq_length']['text']
        enc, el, _ = O.listener_fwd(b['inputs']['features'].astype(np.float64), b['input_seq_length']['features'],
                                    ref.layers)
        lg, ll, _ = O.speller_fwd(enc, el, y, yl, ref.p, 'vanilla')
        att = XS.average(lg, y, ll, yl, 0.1)[0].mean()
        nll, _ = O.ctc_loss(O.linear_fwd(enc, ref.W, ref.b), el, y, yl - 1)
        want.append((1 - LAM) * att + LAM * nll.mean())
    assert abs(loss - np.mean(want)) / np.mean(want) < 1e-4, (loss, want)
    assert tr.adam_step == 1
    moved = tr.model.store.state_dict()
    assert np.abs(moved[HEAD_W] - st0[HEAD_W]).max() > 0          # the head is trained


def test_an_utterance_whose_targets_do_not_fit_raises_the_ctc_error():
    from nabu_amd.neuralnetworks.trainers import loss_functions
    d = SyntheticData(2, 16, 40, min_labels=2, max_labels=3, eos=True, time_reduction=8, seed=1)
    tr = trainer(d, **{'trainer.ctc_weight': LAM, 'trainer.batch_size': 2, 'encoder.num_units': 16})
    batch = d.batch(0)
    batch['targets']['text'] = np.array([[0, 0, 0, 39], [0, 0, 0, 39]], np.int32)     # 3 repeats need 5 frames of 2
    batch['target_seq_length']['text'] = np.array([4, 4], np.int32)
    tr.step(tr.to_device(batch))
    with pytest.raises(Exception, match='Not enough time'):
        loss_functions.check_status()


def test_validation_loss_is_the_plain_attention_loss():
    d = data()
    over = {'trainer.ctc_weight': LAM, 'evaluator.batch_size': B, 'evaluator.numbatches': 1}
    tr = trainer(d, **over)
    tr._create_graph()
    got = tr.validation_loss()
    ref = Ref(tr.model.store.state_dict())
    _, att, _ = ref.step(d.validation(1, B).batch(0))
    assert abs(got - att) / att < 1e-4, (got, att)


def test_two_ranks_on_one_gpu_stay_bit_identical(tmp_path):
    """two real ranks sharing the device, flat and bucketed exchange, 3 updates with ctc_weight = 0.3: the replicas end
    bit-identical, the two exchanges agree, the head is trained and its variables travel in the decoder's bucket"""
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'joint_ctc_two_ranks.py')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', LOCAL_WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen([sys.executable, script, str(tmp_path)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = np.load(str(tmp_path / 'rank0.npz')), np.load(str(tmp_path / 'rank1.npz'))
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for mode in ('flat', 'buckets'):
        for f in ('flat', 'adam_m', 'adam_v'):
            name = mode + '/' + f
            np.testing.assert_array_equal(bits(a[name]), bits(b[name]), err_msg=name)              # rank 0 == rank 1
            np.testing.assert_array_equal(bits(a[name]), bits(a['flat/' + f]), err_msg=name)       # both exchanges
        assert not np.array_equal(a[mode + '/losses'], b[mode + '/losses'])      # the ranks saw different batches
        assert np.isfinite(a[mode + '/losses']).all() and len(a[mode + '/losses']) == 3
        assert np.abs(a[mode + '/head'] - a[mode + '/head_initial']).max() > 0    # the head moved
    assert list(a['buckets/head_buckets']) == ['decoder']


def test_beam_search_decoder_with_the_key_runs_the_head_and_the_joint_search():
    """through decoders/beam_search_decoder.py on a model with a head: with ctc_weight = 0.3 in its conf the decoder
    returns what rnn_decoder.beam_search returns for the head's logits and that weight, and not what it returns without
    the key — which is the plain search, bit for bit, head or no head"""
    import configparser
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.decoders import beam_search_decoder
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    d = data()
    tr = trainer(d, **{'trainer.ctc_weight': LAM})
    for s in range(3):                                   # a few updates: the head's bias leaves zero
        tr.step(tr.to_device(d.batch(s)))
    b = tr.to_device(d.batch(5))
    alphabet = ' '.join('s%d' % i for i in range(list(tr.model.output_dims.values())[0]))

    def decoder(**extra):
        conf = configparser.ConfigParser()
        conf.read_dict({'decoder': dict({'decoder': 'beam_search_decoder', 'alphabet': alphabet, 'max_steps': '6',
                                         'beam_width': '4', 'length_penalty': '0.0', 'temperature': '1.0',
                                         'visualize_alignments': 'False'}, **extra)})
        return beam_search_decoder.BeamSearchDecoder(conf, tr.model)
    plain = decoder()(b['inputs'], b['input_seq_length'])['text']
    joint = decoder(ctc_weight=str(LAM))(b['inputs'], b['input_seq_length'])['text']
    model = tr.model
    with torch.no_grad(), vs.as_default(model.store):
        encoded, lens = model.encoder(inputs=b['inputs'], input_seq_length=b['input_seq_length'], is_training=False)
        with vs.variable_scope(model.decoder.scope):
            cell = model.decoder.create_cell(encoded, lens, False)
            head, head_len = model.decoder.ctc_logits(encoded, lens)
            args = (cell, [encoded['features']], [lens['features']], 4, 6, 0.0, 1.0, False)
            want_plain = rnn_decoder.beam_search(*args)
            want_joint = rnn_decoder.beam_search(*args, ctc_logits=head, ctc_weight=LAM)
    assert tuple(head.shape) == tuple(encoded['features'].shape[:2]) + (40,) and head_len is lens['features']
    for got, want in ((plain, want_plain), (joint, want_joint)):
        for a, w in zip(got[:3], want[:3]):
            assert torch.equal(a, w)
    assert not torch.equal(joint[2], plain[2]) and torch.isfinite(joint[2][:, 0]).all()
