"""CPU: the names and keys of the transducer's forced alignment — nabu_transducer_align in the header and the binding,
decoder = transducer_alignment_decoder, emission_times in transducer_decoder — what refuses them at construction, and
that transducer_decoder without the key makes the calls it always made."""
import configparser
import glob
import os

import numpy as np
import pytest
import torch

from nabu_amd import _hip, ops, recipes
from nabu_amd import variables as vs
from nabu_amd.neuralnetworks.decoders import decoder_factory, transducer_alignment_decoder, transducer_decoder
from nabu_amd.neuralnetworks.models.ed_decoders import transducer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('nabu_transducer_align_ws_bytes', 'nabu_transducer_align_lds_bytes', 'nabu_transducer_align')


def _net():
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': {'decoder': 'transducer', 'num_units': '8'}})
    return transducer.Transducer(conf, {'text': 5}, None)


class Model(object):
    decoder, output_names, output_dims = _net(), ['text'], {'text': 5}


class NotTransducer(object):
    decoder, output_names, output_dims = object(), ['text'], {'text': 5}


def _conf(name, **keys):
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': name, 'text_alphabet': 'a b c d'}, **keys)})
    return conf


def test_the_symbols_are_in_the_header_and_in_the_binding():
    header = open(os.path.join(ROOT, 'include', 'nabu_hip.h')).read()
    for name in NEW:
        assert name + '(' in header and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES['nabu_transducer_align'][1]) == 18
    assert 'NABU_TRANSDUCER_ALIGN_WORKGROUP' in header and hasattr(ops, 'transducer_align')


def test_the_factory_and_the_defaults_file():
    cls = decoder_factory.factory('transducer_alignment_decoder')
    assert cls is transducer_alignment_decoder.TransducerAlignmentDecoder and cls.needs_targets is True
    d = cls(_conf('transducer_alignment_decoder'), Model())
    assert (d.blank_symbol, d.frame_seconds, d.raise_on_misfit) == ('_', 0.0, False)
    assert d.alphabets == {'text': ['a', 'b', 'c', 'd']}
    d = cls(_conf('transducer_alignment_decoder', frame_seconds='0.01', misfit='raise', blank_symbol='sil'), Model())
    assert (d.blank_symbol, d.frame_seconds, d.raise_on_misfit) == ('sil', 0.01, True)
    with pytest.raises(Exception, match='validate'):
        d.update_evaluation_loss([0.0], {}, {}, {})
    with pytest.raises(ValueError, match='targets='):
        d({}, {})


@pytest.mark.parametrize('keys,match', [
    ({'lm_file': 'x'}, 'lm_file'), ({'lm_weight': '1'}, 'lm_weight'), ({'insertion_bonus': '1'}, 'insertion_bonus'),
    ({'ctc_weight': '0.3'}, 'ctc_weight'), ({'frame_seconds': '-1'}, 'frame_seconds'), ({'frame_seconds': 'x'}, 'frame_seconds'),
    ({'frame_seconds': 'inf'}, 'frame_seconds'), ({'misfit': 'ignore'}, 'misfit'),
])
def test_the_alignment_decoder_refuses_at_construction(keys, match):
    with pytest.raises(ValueError, match=match):
        transducer_alignment_decoder.TransducerAlignmentDecoder(_conf('transducer_alignment_decoder', **keys), Model())


def test_the_alignment_decoder_refuses_other_models_and_a_missing_alphabet():
    with pytest.raises(ValueError, match='decoder = transducer'):
        transducer_alignment_decoder.TransducerAlignmentDecoder(_conf('transducer_alignment_decoder'), NotTransducer())
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': {'decoder': 'transducer_alignment_decoder'}})
    with pytest.raises(ValueError, match='text_alphabet'):
        transducer_alignment_decoder.TransducerAlignmentDecoder(conf, Model())


def test_emission_times_and_what_stays_refused():
    make = lambda **k: transducer_decoder.TransducerDecoder(_conf('transducer_decoder', max_steps='7', **k), Model())
    d = make()
    assert d.emission_times is False and d.frame_seconds == 0.0
    assert make(emission_times='False').emission_times is False
    d = make(emission_times='True')
    assert d.emission_times is True and d.frame_seconds == 0.0
    assert make(emission_times='True', frame_seconds='0.04').frame_seconds == 0.04
    assert 'timestamps' in transducer_decoder.REFUSED and 'frame_seconds' in transducer_decoder.REFUSED
    with pytest.raises(ValueError, match='emission_times'):
        make(emission_times='yes')
    with pytest.raises(ValueError, match='frame_seconds'):
        make(frame_seconds='0.04')
    with pytest.raises(ValueError, match='frame_seconds'):
        make(emission_times='False', frame_seconds='0.04')
    with pytest.raises(ValueError, match='frame_seconds'):
        make(emission_times='True', frame_seconds='-2')
    for key in ('timestamps', 'lm_file', 'ctc_weight'):
        with pytest.raises(ValueError, match=key):
            make(emission_times='True', **{key: 'True'})


def test_the_key_is_in_no_defaults_file_and_no_shipped_cfg():
    files = glob.glob(os.path.join(ROOT, 'nabu_amd', '**', 'defaults', '*.cfg'), recursive=True) + \
        glob.glob(os.path.join(recipes.RECIPES, '**', '*.cfg'), recursive=True)
    assert len(files) > 20
    for path in files:
        assert 'emission_times' not in open(path).read(), path
    defaults = open(os.path.join(ROOT, 'nabu_amd', 'neuralnetworks', 'decoders', 'defaults',
                                 'transduceralignmentdecoder.cfg')).read()
    for line in ('blank_symbol = _', 'frame_seconds = 0', 'misfit = report'):
        assert line in defaults


class _FakeModel(object):
    """a model whose call returns fixed f on the CPU; the prediction network is replaced by recorders"""
    output_names, output_dims = ['text'], {'text': 5}

    def __init__(self, log):
        self.decoder, self.store, self.log = _net(), vs.VariableStore(device='cpu'), log
        self.decoder.predict_start = lambda o, B, dev: log.append(('predict_start', o, B)) or {}
        self.decoder.predict_step = lambda state, last_id, emit: log.append(('predict_step',)) or torch.zeros(2, 5)
        self.decoder.predict_sequence = lambda o, labels, lens: log.append(('predict_sequence', tuple(labels.shape))) or \
            torch.zeros(2, labels.shape[1] + 1, 5)

    def __call__(self, inputs, input_seq_length, targets, target_seq_length, is_training):
        self.log.append(('model', targets, is_training))
        return {'text': torch.zeros(2, 3, 5)}, {'text': torch.tensor([3, 2], dtype=torch.int32)}


def _run(monkeypatch, recognised=(2, 0), **keys):
    log = []

    def greedy(it, f, g_row, lens, t_pos, out_len, ids, emit, last_id, score):
        log.append(('greedy_step', it))
        t_pos.copy_(lens)                                   # every row is finished at the first poll
        out_len.copy_(torch.tensor(recognised, dtype=torch.int32))
        ids.fill_(-1)
        ids[0, :recognised[0]] = torch.tensor([1, 3][:recognised[0]], dtype=torch.int32)
        score.zero_()

    def align(f, g, enc_len, labels, label_len, raise_on_status=False):
        log.append(('transducer_align', tuple(f.shape), tuple(g.shape), None if labels is None else tuple(labels.shape)))
        L = g.shape[1] - 1
        return (torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, L, dtype=torch.int32), torch.zeros(2, L),
                torch.zeros(2), torch.zeros(1, dtype=torch.int32))
    monkeypatch.setattr(ops, 'transducer_greedy_step', greedy)
    monkeypatch.setattr(ops, 'transducer_align', align)
    model = _FakeModel(log)
    dec = transducer_decoder.TransducerDecoder(_conf('transducer_decoder', max_steps='40', **keys), model)
    out = dec({'features': None}, {'features': None})
    return log, out, dec


def test_without_the_key_the_decoder_makes_the_calls_it_always_made(monkeypatch, tmp_path):
    log, out, dec = _run(monkeypatch)
    names = [entry[0] for entry in log]
    assert names[:3] == ['model', 'predict_start', 'predict_step'] and log[0][1:] == ([], False)
    assert names[3:] == ['greedy_step', 'predict_step'] * transducer_decoder.POLL          # up to the first poll
    assert 'transducer_align' not in names and 'predict_sequence' not in names
    assert len(out['text']) == 2 and out['text'][1].tolist() == [2, 0]
    dec.write(out, str(tmp_path), ['u0', 'u1'])
    assert sorted(os.listdir(str(tmp_path))) == ['text']

    log2, out2, dec2 = _run(monkeypatch, emission_times='True', frame_seconds='0.5')
    names2 = [entry[0] for entry in log2]
    assert names2[:len(names)] == names                       # the search itself is the same calls
    assert names2[len(names):] == ['predict_sequence', 'transducer_align'] and names2.count('model') == 1
    assert log2[-2] == ('predict_sequence', (2, 2)) and log2[-1] == ('transducer_align', (2, 3, 5), (2, 3, 5), (2, 2))
    ids, lens, seg, conf, score = out2['text']
    assert torch.equal(ids, out['text'][0]) and torch.equal(lens, out['text'][1])
    assert tuple(seg.shape) == (2, 40, 2) and tuple(conf.shape) == (2, 40) and tuple(score.shape) == (2,)
    # both labels of row 0 at frame 0 (the fake alignment): [0,1) by the one-frame minimum, then [0,3) to the end
    assert seg[0, :2].tolist() == [[0, 1], [0, 3]] and bool((seg[0, 2:] == -1).all()) and bool((seg[1] == -1).all())
    out_dir = tmp_path / 'timed'
    out_dir.mkdir()
    dec2.write(out2, str(out_dir), ['u0', 'u1'])
    assert sorted(os.listdir(str(out_dir))) == ['text', 'text.ctm']
    assert open(str(out_dir / 'text.ctm')).read().splitlines() == ['u0 1 0.000 0.500 b 1.0000', 'u0 1 0.000 1.500 d 1.0000']


def test_emission_times_when_nothing_was_recognised(monkeypatch, tmp_path):
    """every row of the batch without a label: U1 = 1, no labels operand, empty ctm, the text file as ever"""
    log, out, dec = _run(monkeypatch, recognised=(0, 0), emission_times='True')
    assert log[-2] == ('predict_sequence', (2, 0)) and log[-1] == ('transducer_align', (2, 3, 5), (2, 1, 5), None)
    ids, lens, seg, conf, score = out['text']
    assert lens.tolist() == [0, 0] and bool((ids == -1).all())
    assert tuple(seg.shape) == (2, 40, 2) and bool((seg == -1).all()) and bool((conf == 0).all())
    assert bool(torch.isfinite(score).all())
    dec.write(out, str(tmp_path), ['u0', 'u1'])
    assert open(str(tmp_path / 'text')).read() == 'u0 \nu1 \n' and open(str(tmp_path / 'text.ctm')).read() == ''


def test_predict_sequence_without_labels_reads_the_start_symbol_only(monkeypatch):
    """the real Transducer.predict_sequence on [B,0] targets: one step, the start symbol, g [B,1,C]"""
    from nabu_amd import ops as hip
    from nabu_amd.neuralnetworks.models.ed_decoders import dnn_decoder
    seen = {}

    def fake_tf(layers, C, targets, tsl):
        seen.update(C=C, targets=tuple(targets.shape), lens=tsl.host.tolist())
        return torch.zeros(targets.shape[1] + 1, targets.shape[0], 8)
    net = _net()
    monkeypatch.setattr(net, '_teacher_forced', fake_tf)
    monkeypatch.setattr(dnn_decoder, 'linear', lambda x, C, scope: torch.zeros(x.shape[0], x.shape[1], C))
    with vs.as_default(vs.VariableStore(device='cpu')):
        g = net.predict_sequence('text', torch.zeros((2, 0), dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    assert tuple(g.shape) == (2, 1, 5) and seen == dict(C=5, targets=(2, 0), lens=[0, 0])
    # and what _teacher_forced makes of it before its first kernel: ids [1,B] of the start symbol, seq_len 1
    ids = torch.cat([torch.full((1, 2), 4, dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32).t().clamp(0, 4)], 0)
    assert ids.tolist() == [[4, 4]]


def test_emission_segments_convention():
    seg = transducer_alignment_decoder.emission_segments
    frame = torch.tensor([[0, 0, 2, 5], [1, 4, -1, -1], [-1, -1, -1, -1]], dtype=torch.int32)
    got = seg(frame, torch.tensor([4, 2, 0], dtype=torch.int32), torch.tensor([6, 5, 3], dtype=torch.int32))
    assert got.dtype == torch.int32
    assert got.tolist() == [[[0, 1], [0, 2], [2, 5], [5, 6]], [[1, 4], [4, 5], [-1, -1], [-1, -1]], [[-1, -1]] * 4]
    assert tuple(seg(torch.zeros((2, 0), dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                     torch.ones(2, dtype=torch.int32)).shape) == (2, 0, 2)
    # a rejected row (frame -1 although label_len says 2) gets no segments
    got = seg(torch.tensor([[-1, -1]], dtype=torch.int32), torch.tensor([2], dtype=torch.int32), torch.tensor([4], dtype=torch.int32))
    assert got.tolist() == [[[-1, -1], [-1, -1]]]
    assert np.all(np.diff(np.array([s[0] for s in seg(frame, torch.tensor([4, 2, 0]), torch.tensor([6, 5, 3]))[0].tolist()])) >= 0)
