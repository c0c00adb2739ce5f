"""GPU tests of the sampled decode (the reference's RandomDecoder): the step kernel nabu_sample_advance on its own, the
sampling mode of the decode loop (nabu_speller_sample, nabu_speller_multi_sample) and the decoder class through the
recipe API.

No new oracle for the loop: the sampled sequences are fed back as targets to the TRAINING forward pass
(nabu_speller_fwd, sample_prob 0), whose kernels the goldens cover; its logits must reproduce every sampled id through
nabu_sample_ids at the step's offset, and their cross-entropy must be the loop's nll.

Draws against the host follow the rule of tests/test_hip_sampling.py (DrawStats, near_boundary_limit): exact outside a
band of 1e-5 * total around a CDF boundary, and few rows inside one."""
import configparser
import os

import numpy as np
import pytest
import torch

from oracle import decode_oracle as D
from oracle import philox as P
from nabu_amd import recipes
from tests import random_decoder_ref as R
from tests.test_hip_multi_speller import NAMES, make_decoder
from tests.test_hip_sampling import DrawStats, near_boundary_limit, _logits

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# the bar of tests/test_hip_multi_speller.py for one search through both entry points (BEAM_BOUND; alignments 2e-5)
ENTRY_BOUND = 2e-4
LOGIT_BOUND = 2e-5        # the logits of the step chain against float64 in tests/test_hip_speller.py


def t32(a):
    return torch.tensor(np.asarray(a), device=DEV)


def fresh(B, S):
    return (torch.zeros((B, S), dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV),
            torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------- the step kernel


@pytest.mark.parametrize('C', [9, 40, 64, 256])
def test_step_draws_equal_sample_ids_and_match_the_host(C):
    """B = 300 rows (rows above 255), three logits families, a 64-bit seed and offset: next_ids is nabu_sample_ids at
    prob = 1 bit for bit — also in rows that were finished before the step — and follows the host's float64 draw"""
    from nabu_amd import ops
    B, S = 300, 3
    rng = np.random.default_rng(2000 + C)
    st = DrawStats(C)
    teacher = t32(np.zeros(B, np.int32))
    for k, kind in enumerate(('dominant', 'uniform', 'spread')):
        lg = _logits(kind, B, C, rng)
        lgd = t32(lg)
        seed, offset = ((7, 3), (12345, (5 << 32) + 1000003 * 9 + 4), ((1 << 40) + 3, 77))[k]
        seq, lengths, finished, nll = fresh(B, S)
        finished[::7] = 1
        lengths[::7] = 1
        next_ids, _ = ops.sample_advance(lgd, seed, offset, 1, seq, lengths, finished, nll)
        want = ops.sample_ids(lgd, 1.0, seed, offset, teacher)
        np.testing.assert_array_equal(next_ids.cpu().numpy(), want.cpu().numpy())
        sel = st.add(next_ids.cpu().numpy(), lg, 1.0, seed, offset, np.zeros(B, np.int64))
        assert sel.all()
        # what the step wrote is the draw where the row was running, and nothing where it was not
        ids, seq = next_ids.cpu().numpy(), seq.cpu().numpy()
        was = np.arange(B) % 7 == 0
        np.testing.assert_array_equal(seq[:, 1], np.where(was, 0, ids))
        assert not seq[:, [0, 2]].any() and not nll.cpu().numpy()[was].any()
        np.testing.assert_array_equal(finished.cpu().numpy(), (was | (ids == C - 1)).astype(np.int32))
    st.check('sample_advance')


@pytest.mark.parametrize('ends', [(0, 2, 4, None), (1, 3, 3, 0)])
def test_step_bookkeeping_with_forced_end_tokens(ends):
    """+50 on class C - 1 at the step a row is to end, -50 on it otherwise: lengths, finished, zeros after the end, nll
    frozen after the end (same bits), lengths = max_steps for the row that never ends, and all_finished exactly from
    the step at which the last row ends"""
    from nabu_amd import ops
    B, C, S = len(ends), 9, 6
    rng = np.random.default_rng(5)
    seq, lengths, finished, nll = fresh(B, S)
    ref = R.State(B, S)
    last = max(S - 1 if e is None else e for e in ends)
    frozen = {}
    for t in range(S):
        lg = rng.normal(size=(B, C)).astype(np.float32)
        for b, e in enumerate(ends):
            if e == t:
                lg[b] = 0.0
                lg[b, C - 1] = 50.0
            else:
                lg[b, C - 1] = -50.0
        next_ids, all_fin = ops.sample_advance(t32(lg), 11, 100 + t, t, seq, lengths, finished, nll)
        ids = next_ids.cpu().numpy()
        for b, e in enumerate(ends):
            assert (ids[b] == C - 1) == (e == t), (t, b, ids[b])
        want_all = ref.advance(t, lg, ids)
        assert int(all_fin.item()) == want_all == int(t >= last), t
        np.testing.assert_array_equal(seq.cpu().numpy(), ref.sequences)
        np.testing.assert_array_equal(lengths.cpu().numpy(), ref.lengths)
        np.testing.assert_array_equal(finished.cpu().numpy(), ref.finished)
        got = nll.cpu().numpy()
        np.testing.assert_allclose(got, ref.nll, rtol=1e-6, atol=1e-30)
        for b in range(B):
            if ref.finished[b]:
                assert frozen.setdefault(b, got[b]) == got[b], (t, b)
    want_len = [S if e is None else e + 1 for e in ends]
    np.testing.assert_array_equal(lengths.cpu().numpy(), want_len)
    for b, n in enumerate(want_len):
        assert not ref.sequences[b, n:].any()


def test_step_nll_against_float64():
    """B = 33, C = 40, 12 steps of fresh logits: nll against the float64 sum of logsumexp - logit over the ids the
    kernel drew, to 1e-6 relative per row — what tests/test_hip_ops.py allows a cross-entropy loss"""
    from nabu_amd import ops
    B, C, S = 33, 40, 12
    rng = np.random.default_rng(33)
    seq, lengths, finished, nll = fresh(B, S)
    ref = R.State(B, S)
    for t in range(S):
        lg = (2.0 * rng.normal(size=(B, C))).astype(np.float32)
        next_ids, _ = ops.sample_advance(t32(lg), 21, 5000 + t, t, seq, lengths, finished, nll)
        ref.advance(t, lg, next_ids.cpu().numpy())
    np.testing.assert_array_equal(lengths.cpu().numpy(), ref.lengths)
    assert (ref.lengths == S).any() and (ref.lengths < S).any() and ref.nll.min() > 0
    rel = np.abs(nll.cpu().numpy() - ref.nll) / ref.nll
    print('nll against float64: largest relative error %.3g (row of %d steps)' % (rel.max(), ref.lengths[rel.argmax()]))
    assert rel.max() < 1e-6


def test_step_rejects_a_step_outside_the_sequence():
    from nabu_amd import _hip, ops
    seq, lengths, finished, nll = fresh(2, 3)
    with pytest.raises(_hip.NabuHipError):
        ops.sample_advance(t32(np.zeros((2, 4), np.float32)), 1, 1, 3, seq, lengths, finished, nll)


# ------------------------------------------------------------------------------------------------- the loop


class Case(object):
    """a small Speller over M memories with its own variable store; sample() and teacher() run it on the GPU"""

    def __init__(self, attention, nl=2, B=5, Tes=(13,), Es=(8,), U=16, C=9, S=10, enc_lens=None, seed=5):
        from nabu_amd import variables as vs
        K, F = (3, 2) if attention == 'location_aware' else (0, 0)
        self.dec = make_decoder(attention, 'softmax', nl, U, K, F, C, extra={'decoder.sample_prob': 0.0})
        self.store = vs.VariableStore(seed=seed)
        rng = np.random.default_rng(seed)
        self.B, self.C, self.S, self.M = B, C, S, len(Tes)
        self.enc_lens = enc_lens or [np.array([Te, 0, Te // 2, Te - 1, 3][:B], np.int32) for Te in Tes]
        self.encs = []
        for Te, E, el in zip(Tes, Es, self.enc_lens):
            e = rng.normal(size=(B, Te, E)).astype(np.float32)
            self.encs.append(e * (np.arange(Te)[None, :, None] < el[:, None, None]))

    def _inputs(self):
        from nabu_amd.autodiff import SeqLen
        enc = {NAMES[m]: t32(self.encs[m]) for m in range(self.M)}
        lens = {NAMES[m]: SeqLen(self.enc_lens[m].astype(np.int32), torch.device(DEV)) for m in range(self.M)}
        return enc, lens

    def sample(self, seed, offset, with_alignments=True):
        """(sequences [B, steps], lengths, nll, [alignments per memory]) as numpy"""
        from nabu_amd import variables as vs
        from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
        enc, lens = self._inputs()
        with torch.no_grad(), vs.as_default(self.store), vs.variable_scope('Speller'):
            cell = self.dec.create_cell(enc, lens, False)
            seq, lengths, nll, al = rnn_decoder.sample(cell, list(enc.values()), list(lens.values()), self.S, seed, offset,
                                                       with_alignments)
        if with_alignments:
            al = [a.cpu().numpy() for a in (al if isinstance(al, list) else [al])]
        return seq.cpu().numpy(), lengths.cpu().numpy(), nll.cpu().numpy(), al

    def teacher(self, seq, lengths):
        """logits [B, max(lengths), C] of the training forward pass fed `seq` as targets, dec_len = lengths"""
        from nabu_amd import variables as vs
        from nabu_amd.autodiff import SeqLen, Tape
        enc, lens = self._inputs()
        with torch.no_grad(), vs.as_default(self.store), Tape():
            logits, _, _ = self.dec(enc, lens, {'text': t32(seq.astype(np.int32))},
                                    {'text': SeqLen(lengths.astype(np.int32), torch.device(DEV))}, False)
        return logits['text']


def check_against_the_training_chain(case, seq, lengths, nll, seed, offset0):
    """the teacher-forced logits reproduce the sampled ids through nabu_sample_ids at offset0 + t and give the nll"""
    from nabu_amd import ops
    B, S, C = case.B, case.S, case.C
    assert seq.shape[0] == B and seq.shape[1] == lengths.max() <= S
    assert lengths.min() >= 1
    for b in range(B):
        n = lengths[b]
        assert not seq[b, n:].any() and not (seq[b, :n - 1] == C - 1).any()
        assert seq[b, n - 1] == C - 1 or n == S
    logits = case.teacher(seq, lengths)
    teacher = t32(np.zeros(B, np.int32))
    for t in range(logits.shape[1]):
        rows = t < lengths
        got = ops.sample_ids(logits[:, t].contiguous(), 1.0, seed, offset0 + t, teacher).cpu().numpy()
        np.testing.assert_array_equal(got[rows], seq[rows, t], err_msg='step %d' % t)
    # every term logsumexp - logit moves by at most twice the error of the logits
    want = R.sample_nll(logits.cpu().numpy(), seq, lengths)
    print('lengths %s, nll against the teacher-forced cross-entropy: %.3g' % (lengths, np.abs(nll - want).max()))
    np.testing.assert_allclose(nll, want, rtol=1e-6, atol=2 * LOGIT_BOUND * S)
    return logits


@pytest.mark.parametrize('attention', ['vanilla', 'location_aware'])
def test_sampled_sequences_reproduce_under_the_training_chain(attention):
    """B = 5 (one utterance without frames), Te = 13, E = 8, U = 16, C = 9, two layers, max_steps = 10"""
    case = Case(attention)
    seed, offset0 = 17, 4 * 1000003
    seq, lengths, nll, al = case.sample(seed, offset0)
    check_against_the_training_chain(case, seq, lengths, nll, seed, offset0)
    a = al[0]
    assert a.shape == (5, seq.shape[1], 13)
    for b in range(5):
        sums = a[b, :lengths[b]].sum(-1)
        np.testing.assert_allclose(sums, 0.0 if case.enc_lens[0][b] == 0 else 1.0, atol=1e-5)
        assert not a[b, :, case.enc_lens[0][b]:].any()


@pytest.mark.parametrize('attention,Te', [('vanilla', 13), ('location_aware', 13), ('location_aware', 40)])
def test_one_memory_through_both_sample_entry_points(attention, Te, monkeypatch):
    """the same decoder, memory, seed and offset through nabu_speller_sample (nabu_attn_fwd) and through
    nabu_speller_multi_sample with M = 1 (multi_attn_fwd); 40 frames run both attention kernels frame-sliced, with
    partials.  The two kernels may round differently: a row may part where its draw lies within the boundary band of
    the host's CDF (and on a class of that band), not elsewhere"""
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    # (the 40-frame case without the utterance of length 0)
    case = Case(attention, Tes=(Te,), enc_lens=[np.array([40, 20, 33, 39, 3], np.int32)] if Te == 40 else None)
    seed, offset0 = 29, 6 * 1000003
    called, fn = [], rnn_decoder._Binding.fn
    monkeypatch.setattr(rnn_decoder._Binding, 'fn', lambda self, name: (called.append(self.prefix + name), fn(self, name))[1])
    seq0, len0, nll0, al0 = case.sample(seed, offset0)
    monkeypatch.setattr(rnn_decoder, '_force_multi', True)
    seq1, len1, nll1, al1 = case.sample(seed, offset0)
    monkeypatch.setattr(rnn_decoder, '_force_multi', False)
    assert called == ['nabu_speller_sample_ws_bytes', 'nabu_speller_sample', 'nabu_speller_multi_sample_ws_bytes',
                      'nabu_speller_multi_sample']
    same = np.ones(case.B, bool)
    n = min(seq0.shape[1], seq1.shape[1])
    parted = [b for b in range(case.B) if seq0.shape != seq1.shape or (seq0[b, :n] != seq1[b, :n]).any()]
    if parted:
        logits = case.teacher(seq0, len0).cpu().numpy()
        for b in parted:
            t = int(np.argmax(seq0[b, :n] != seq1[b, :n]))
            _, _, margin, bounds = P.reference_draw(logits[:, t].astype(np.float64), 1.0, seed, offset0 + t,
                                                    np.zeros(case.B, np.int64))
            assert margin[b] <= 1e-5 and bounds[b, 0] <= min(seq0[b, t], seq1[b, t]) and \
                max(seq0[b, t], seq1[b, t]) <= bounds[b, 1], (b, t, margin[b])
            same[b] = False
        assert len(parted) <= near_boundary_limit(case.C, int(len0.sum())), parted
    print('%d rows parted; nll diff %.3g, alignments diff %.3g' % (
        len(parted), np.abs(nll1 - nll0)[same].max(), np.abs(al1[0][:, :n] - al0[0][:, :n])[same].max()))
    np.testing.assert_array_equal(seq1[same, :n], seq0[same, :n])
    np.testing.assert_array_equal(len1[same], len0[same])
    np.testing.assert_allclose(nll1[same], nll0[same], rtol=ENTRY_BOUND, atol=ENTRY_BOUND)
    np.testing.assert_allclose(al1[0][same, :n], al0[0][same, :n], atol=2e-5)


def test_two_memories():
    """M = 2, memories of different Te and E: one alignments tensor per memory whose rows sum to 1 below `lengths`;
    the sampled ids and the nll reproduce under nabu_speller_multi_fwd"""
    case = Case('vanilla', nl=1, B=3, Tes=(6, 9), Es=(8, 12), U=16, C=5, S=6,
                enc_lens=[np.array([6, 3, 5], np.int32), np.array([4, 9, 1], np.int32)])
    seed, offset0 = 3, 9 * 1000003
    seq, lengths, nll, al = case.sample(seed, offset0)
    check_against_the_training_chain(case, seq, lengths, nll, seed, offset0)
    assert len(al) == 2 and [a.shape for a in al] == [(3, seq.shape[1], 6), (3, seq.shape[1], 9)]
    for m, a in enumerate(al):
        for b in range(3):
            np.testing.assert_allclose(a[b, :lengths[b]].sum(-1), 1.0, atol=1e-5)
            assert not a[b, :, case.enc_lens[m][b]:].any()


def test_identical_calls_give_identical_bits_and_the_offset_matters():
    case = Case('location_aware')
    first, second = case.sample(41, 1000003), case.sample(41, 1000003)
    for a, b in zip(first[:3] + tuple(first[3]), second[:3] + tuple(second[3])):
        np.testing.assert_array_equal(a, b)
    other = case.sample(41, 2 * 1000003)
    assert other[0].shape != first[0].shape or (other[0] != first[0]).any()
    without = case.sample(41, 1000003, with_alignments=False)
    assert without[3] is None
    np.testing.assert_array_equal(without[0], first[0])
    np.testing.assert_array_equal(without[2], first[2])


def test_sample_entry_points_validate_on_the_host():
    import ctypes
    from nabu_amd import _hip
    lib = _hip.lib()
    d = _hip.BeamDesc(ctypes.sizeof(_hip.BeamDesc), 5, 13, 8, 16, 9, 2, 0, 0, 0, 0, 1, 10, 0.0, 0.0)
    assert lib.nabu_speller_sample_ws_bytes(ctypes.byref(d)) > 0          # temperature is ignored
    assert lib.nabu_speller_beam_ws_bytes(ctypes.byref(d)) == 0
    d.beam_width = 2
    assert lib.nabu_speller_sample_ws_bytes(ctypes.byref(d)) == 0 and b'beam_width must be 1' in lib.nabu_last_error()


# ------------------------------------------------------------------------------------------- the recipe level


def test_random_decoder_and_evaluator_through_the_recipe_api(tmp_path):
    """a shrunken cfg3 model on synthetic data: DecoderEvaluator with decoder = random_decoder gives the error rate of
    sequences[:, :lengths - 1] against the references; ops.set_seed makes the decode reproducible and every call
    takes max_steps offsets of the global stream"""
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.evaluators import evaluator_factory
    from nabu_amd.neuralnetworks.models.model import Model
    from nabu_amd.processing.synthetic import SyntheticData
    mc, tc, _ = recipes.load_recipe('cfg3_las_vanilla', **{'encoder.num_units': 32, 'decoder.num_units': 32})
    model = Model(mc, int(tc.get('trainer', 'trainlabels')), None, seed=4)
    data = SyntheticData(4, 64, 40, min_frames=40, min_labels=2, max_labels=6, eos=True, time_reduction=8, seed=78)
    alphabet = ' '.join('s%d' % i for i in range(64))
    conf = configparser.ConfigParser()
    conf.read_dict({'evaluator': {'evaluator': 'decoder_evaluator', 'batch_size': '4', 'numbatches': '2',
                                  'targets': 'text'},
                    'decoder': {'decoder': 'random_decoder', 'alphabet': alphabet, 'max_steps': '10'}})
    ev = evaluator_factory.factory('decoder_evaluator')(conf, data, model)
    nops.set_seed(123)
    loss, update, nb = ev.evaluate()
    for i in range(nb):
        update(i)
    assert nops.global_rng().offset == 10 * nb and np.isfinite(loss[0]) and loss[0] >= 0
    nops.set_seed(123)
    errors = targets = 0
    for i in range(nb):
        batch = ev.data.batch(i)
        out = ev.decoder({'features': t32(batch['inputs']['features'])}, {'features': batch['input_seq_length']['features']})
        labels, lengths, logprobs = (x.cpu().numpy() for x in out['text'])
        assert labels.shape[0] == 4 and (lengths >= 1).all() and (logprobs > 0).all()
        for b in range(4):
            tl = batch['target_seq_length']['text'][b]
            errors += D.edit_distance(list(labels[b, :lengths[b] - 1]), list(batch['targets']['text'][b, :tl]))
            targets += tl
    assert abs(loss[0] - errors / targets) < 1e-9
    ev.decoder.write(out, str(tmp_path), ['u%d' % b for b in range(4)])
    lines = open(tmp_path / 'text').read().strip('\n').split('\n')
    assert len(lines) == 4
    assert lines[2].split(' ') == ['u2'] + ['s%d' % j for j in labels[2, :lengths[2]]]


def test_run_decode_writes_one_line_per_utterance(tmp_path):
    """`run decode` on an experiment directory whose recognizer.cfg names the random decoder"""
    from tests.test_data_path import make_dataset
    from nabu_amd.scripts import decode as decode_script
    expdir = str(tmp_path / 'exp')
    os.makedirs(expdir)
    conf, feats, _, _ = make_dataset(str(tmp_path / 'test'), n=7, dim=40, seed=9, min_frames=16)
    mc, tc, _ = recipes.load_recipe('cfg3_las_vanilla', **{'encoder.num_units': 16, 'decoder.num_units': 16})
    alphabet = ['s%d' % i for i in range(64)]
    rc = configparser.ConfigParser()
    rc.read_dict({'recognizer': {'batch_size': '3', 'features': 'trainfbank'},
                  'decoder': {'decoder': 'random_decoder', 'alphabet': ' '.join(alphabet), 'max_steps': '5'}})
    for name, c in (('database.conf', conf), ('model.cfg', mc), ('trainer.cfg', tc), ('recognizer.cfg', rc)):
        with open(os.path.join(expdir, name), 'w') as fid:
            c.write(fid)
    out = decode_script.decode(expdir)
    lines = open(os.path.join(out, 'text')).read().strip('\n').split('\n')
    assert sorted(l.split(' ')[0] for l in lines) == sorted(feats)
    for l in lines:
        labels = l.split(' ')[1:]
        assert 1 <= len(labels) <= 5 and all(s in alphabet for s in labels)
