"""CPU: the decoders' language-model keys (lm_file, lm_weight, insertion_bonus).  They are extension keys: absent from
every defaults file and shipped recipe, off when absent — a decoder without them makes the calls it always made (call
spies, as tests/test_trainer_call_order.py) —, refused with the key named when they make no sense."""
import configparser
import glob
import os

import numpy as np
import pytest
import torch

from nabu_amd.processing import ngram_lm
from tests.test_joint_ctc_keys import _Model, _decoder_conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('lm_file', 'lm_weight', 'insertion_bonus')


def test_keys_are_absent_from_defaults_and_recipes():
    files = glob.glob(os.path.join(ROOT, 'nabu_amd', '**', 'defaults', '*.cfg'), recursive=True) + \
        glob.glob(os.path.join(ROOT, 'config', '**', '*.cfg'), recursive=True)
    assert len(files) > 10
    for f in files:
        text = open(f).read()
        for k in KEYS:
            assert k not in text, (f, k)


def lm_file(tmp_path, alphabet, order=2, name='lm.npz'):
    path = str(tmp_path / name)
    ngram_lm.train([[0, 1], [1, 0, 1]], alphabet, order).save(path)
    return path


# ------------------------------------------------------------------------------------------------ BeamSearchDecoder
def test_beam_search_decoder_keys(tmp_path, monkeypatch):
    from nabu_amd import variables as vs
    from nabu_amd.neuralnetworks.decoders import beam_search_decoder as bsd
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    seen = []
    monkeypatch.setattr(rnn_decoder, 'beam_search', lambda *a, **kw: seen.append((a, kw)) or ('s', 'l', 'sc', None))
    monkeypatch.setattr(vs, 'as_default', lambda store: vs.variable_scope('x'))
    loads = []
    real_load = ngram_lm.load
    monkeypatch.setattr(ngram_lm, 'load', lambda *a, **kw: loads.append(a) or real_load(*a, **kw))
    plain = dict(beam_width=3, max_steps=4, length_penalty=0.0, temperature=1.0, with_alignments=False)
    path = lm_file(tmp_path, ['a', 'b', 'c', 'd'])                   # the model's output dimension is 5 = 4 labels + 1
    # without the keys: the call it always was, nothing loaded
    dec = bsd.BeamSearchDecoder(_decoder_conf(), _Model(False))
    assert dec.lm is None and dec.lm_weight == 0.0
    dec({'features': None}, {'features': None})
    assert seen.pop() == (('cell', ['encoded'], ['lengths']), plain) and loads == []
    # with them: the model object and the weight reach the search; the file is read once, at construction
    dec = bsd.BeamSearchDecoder(_decoder_conf(lm_file=path, lm_weight='0.4'), _Model(False))
    for _ in range(2):
        dec({'features': None}, {'features': None})
        args, kw = seen.pop()
        assert kw == dict(plain, lm=dec.lm, lm_weight=0.4) and kw['lm'].order == 2
    assert len(loads) == 1
    # combined with ctc_weight
    model = _Model(True)
    dec = bsd.BeamSearchDecoder(_decoder_conf(lm_file=path, lm_weight='0.4', ctc_weight='0.3'), model)
    dec({'features': None}, {'features': None})
    assert seen.pop()[1] == dict(plain, ctc_logits='head logits', ctc_weight=0.3, lm=dec.lm, lm_weight=0.4)
    # weight 0 with a file: off
    dec = bsd.BeamSearchDecoder(_decoder_conf(lm_file=path, lm_weight='0'), _Model(False))
    dec({'features': None}, {'features': None})
    assert seen.pop()[1] == plain
    # refusals name the key
    with pytest.raises(ValueError, match='lm_weight needs a language model.*lm_file'):
        bsd.BeamSearchDecoder(_decoder_conf(lm_weight='0.4'), _Model(False))
    for bad in ('-1', 'nan', 'inf', 'x'):
        with pytest.raises(ValueError, match='lm_weight'):
            bsd.BeamSearchDecoder(_decoder_conf(lm_file=path, lm_weight=bad), _Model(False))
    with pytest.raises(ValueError, match='insertion_bonus'):
        bsd.BeamSearchDecoder(_decoder_conf(lm_file=path, insertion_bonus='1'), _Model(False))
    with pytest.raises(ValueError, match='alphabet'):
        bsd.BeamSearchDecoder(_decoder_conf(lm_file=lm_file(tmp_path, ['a', 'b', 'd', 'c'], name='o.npz')), _Model(False))
    with pytest.raises(ValueError, match='num_labels'):
        bsd.BeamSearchDecoder(_decoder_conf(lm_file=lm_file(tmp_path, ['a', 'b', 'c'], name='s.npz')), _Model(False))


def test_beam_search_refuses_a_weight_without_a_model_and_a_bad_weight():
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    with pytest.raises(ValueError, match='lm_weight 0.5 needs a language model'):
        rnn_decoder.beam_search(None, None, None, 3, 4, lm_weight=0.5)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='lm_weight'):
            rnn_decoder.beam_search(None, None, None, 3, 4, lm='lm', lm_weight=bad)


# ------------------------------------------------------------------------------------------------------- CTCDecoder
class _CtcModel(object):
    output_names = ['text']
    output_dims = {'text': 5}

    def __call__(self, inputs, input_seq_length, targets, target_seq_length, is_training):
        return {'text': torch.zeros(2, 3, 5)}, {'text': np.array([3, 2], np.int32)}


def _ctc_conf(**extra):
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': 'ctc_decoder', 'text_alphabet': 'a b c d'}, **extra)})
    return conf


def test_ctc_decoder_keys(tmp_path, monkeypatch):
    from nabu_amd import ops
    from nabu_amd.neuralnetworks.decoders import ctc_decoder as cd
    calls = []
    monkeypatch.setattr(ops, 'ctc_beam_search', lambda lg, ln, W, merge_repeated: calls.append(('plain', W, merge_repeated)) or ('ids', 'len', 'lp'))

    def fused(lg, ln, table, order, weight, bonus, W, merge_repeated):
        calls.append(('lm', table, order, weight, bonus, W, merge_repeated))
        return 'ids', 'len', 'lp'
    monkeypatch.setattr(ops, 'ctc_beam_search_lm', fused)
    path = lm_file(tmp_path, ['a', 'b', 'c', 'd'], order=3)
    dec = cd.CTCDecoder(_ctc_conf(), _CtcModel())
    assert dec.lm is None and dec({}, {}) == {'text': ('ids', 'len')}
    assert calls == [('plain', 100, True)]                            # without the keys: the call it always made
    del calls[:]
    dec = cd.CTCDecoder(_ctc_conf(lm_file=path, lm_weight='0.6', insertion_bonus='-0.25'), _CtcModel())
    dec({}, {})
    dec({}, {})
    assert [c[0] for c in calls] == ['lm', 'lm'] and calls[0][2:] == (3, 0.6, -0.25, 100, True)
    assert calls[0][1] is calls[1][1] and tuple(calls[0][1].shape) == (25, 5)      # one upload per decoder object
    assert cd.CTCDecoder(_ctc_conf(lm_file=path), _CtcModel()).insertion_bonus == 0.0
    with pytest.raises(ValueError, match='lm_weight needs a language model.*lm_file'):
        cd.CTCDecoder(_ctc_conf(lm_weight='0.4'), _CtcModel())
    with pytest.raises(ValueError, match='insertion_bonus needs a language model.*lm_file'):
        cd.CTCDecoder(_ctc_conf(insertion_bonus='0.4'), _CtcModel())
    for key, bads in (('lm_weight', ('-1', 'nan', 'x')), ('insertion_bonus', ('inf', 'nan', 'x'))):
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                cd.CTCDecoder(_ctc_conf(**{'lm_file': path, key: bad}), _CtcModel())
    with pytest.raises(ValueError, match='alphabet'):
        cd.CTCDecoder(_ctc_conf(lm_file=lm_file(tmp_path, ['a', 'b', 'd', 'c'], name='o.npz')), _CtcModel())
    with pytest.raises(ValueError, match='num_labels'):
        cd.CTCDecoder(_ctc_conf(lm_file=lm_file(tmp_path, ['a', 'b'], name='s.npz')), _CtcModel())


# --------------------------------------------------------------------------------- the decoders without a label search
def test_random_and_alignment_decoders_refuse_the_keys():
    from nabu_amd.neuralnetworks.decoders import alignment_decoder, random_decoder
    for cls, base in ((random_decoder.RandomDecoder, {'decoder': 'random_decoder', 'alphabet': 'a b', 'max_steps': '4'}),
                      (alignment_decoder.AlignmentDecoder, {'decoder': 'alignment_decoder', 'prior': 'p.npy'})):
        for key in KEYS:
            conf = configparser.ConfigParser()
            conf.read_dict({'decoder': dict(base, **{key: '1'})})
            with pytest.raises(ValueError, match=key):
                cls(conf, object())
