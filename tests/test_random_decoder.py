"""CPU tests of the RandomDecoder (decoders/random_decoder.py): the factory entry, its defaults, the file it writes and
the error rate it folds in.  The device kernels behind it are tests/test_hip_random_decoder.py."""
import configparser
import os
import types

import numpy as np
import pytest
import torch

from oracle import decode_oracle as D

ALPHABET = 'a b c d <eos>'


def _decoder(extra=None):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': 'random_decoder', 'alphabet': ALPHABET, 'max_steps': '6'}, **(extra or {}))})
    model = types.SimpleNamespace(output_dims={'text': 5})
    return decoder_factory.factory('random_decoder')(conf, model)


def test_factory_gives_the_random_decoder():
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    from nabu_amd.neuralnetworks.decoders.random_decoder import RandomDecoder
    assert decoder_factory.factory('random_decoder') is RandomDecoder
    assert 'random_decoder' in decoder_factory.factory.names()


@pytest.mark.parametrize('name', ['max_decoder', 'threshold_decoder', 'feature_decoder'])
def test_the_other_reference_decoders_still_raise(name):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    with pytest.raises(Exception, match='outside the MI355X hot path'):
        decoder_factory.factory(name)


def test_defaults_load_and_required_keys_are_required():
    """defaults/randomdecoder.cfg has the reference's two keys, both without a default"""
    from nabu_amd.neuralnetworks.decoders import decoder as decoder_mod
    here = os.path.dirname(decoder_mod.__file__)
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(here, 'defaults', 'randomdecoder.cfg'))
    assert sorted(cfg.options('default')) == ['alphabet', 'max_steps']
    dec = _decoder()
    assert dec.alphabet == ALPHABET.split(' ') and int(dec.conf['max_steps']) == 6 and dec.num_targets == 0.0


def test_write_appends_name_and_labels_cut_at_lengths(tmp_path):
    dec = _decoder()
    labels = torch.tensor([[0, 1, 4, 0, 0, 0], [3, 3, 2, 1, 0, 2], [4, 0, 0, 0, 0, 0]], dtype=torch.int32)
    lengths = torch.tensor([3, 6, 1], dtype=torch.int32)
    nll = torch.tensor([1.0, 2.0, 3.0])
    dec.write({'text': (labels, lengths, nll)}, str(tmp_path), ['u0', 'u1', 'u2'])
    dec.write({'text': (labels[:1], lengths[:1], nll[:1])}, str(tmp_path), ['u3'])          # appends
    assert open(tmp_path / 'text').read() == 'u0 a b <eos>\nu1 d d c b a c\nu2 <eos>\nu3 a b <eos>\n'


def test_update_evaluation_loss_folds_the_edit_distance_of_all_but_the_last_label(monkeypatch):
    """sequences[:, :lengths - 1] against the WHOLE references (random_decoder.py:163-185), over the number of
    reference labels.  nabu_edit_distance is a device kernel: here it is replaced by the oracle's Levenshtein distance,
    which also records what it was handed."""
    from nabu_amd import ops
    seen = {}

    def edit_distance(hyp, hyp_len, truth, truth_len):
        seen['hyp_len'], seen['truth_len'] = hyp_len.tolist(), truth_len.tolist()
        return torch.tensor([D.edit_distance(list(h[:n]), list(t[:m])) for h, n, t, m in
                             zip(hyp.tolist(), hyp_len.tolist(), truth.tolist(), truth_len.tolist())], dtype=torch.int32)
    monkeypatch.setattr(ops, 'edit_distance', edit_distance)
    dec = _decoder()
    # row 0 ended with <eos>: [0 1] vs [0 1] -> 0;  row 1 never ended (lengths = max_steps): its last label is dropped,
    # [3 3 2 1 0] vs [3 2 1 0 2 4] -> 3 (one deletion, two insertions);  row 2 drew <eos> at once: [] vs [1 4] -> 2
    labels = torch.tensor([[0, 1, 4, 0, 0, 0], [3, 3, 2, 1, 0, 2], [4, 0, 0, 0, 0, 0]], dtype=torch.int32)
    lengths = torch.tensor([3, 6, 1], dtype=torch.int32)
    refs = np.array([[0, 1, 0, 0, 0, 0], [3, 2, 1, 0, 2, 4], [1, 4, 0, 0, 0, 0]], np.int32)
    ref_len = np.array([2, 6, 2], np.int32)
    loss = [0.0]
    dec.update_evaluation_loss(loss, {'text': (labels, lengths, None)}, {'text': refs}, {'text': ref_len})
    assert seen == {'hyp_len': [2, 5, 0], 'truth_len': [2, 6, 2]}
    assert loss[0] == pytest.approx(5 / 10) and dec.num_targets == 10
    # a second batch, [0 1] vs [0 0] -> 1, folds into the running rate: (5 + 1) / (10 + 2)
    dec.update_evaluation_loss(loss, {'text': (labels[:1], lengths[:1], None)}, {'text': refs[:1, ::-1].copy()},
                               {'text': ref_len[:1]})
    assert D.edit_distance([0, 1], [0, 0]) == 1
    assert loss[0] == pytest.approx(6 / 12) and dec.num_targets == 12
    dec.reset()
    assert dec.num_targets == 0.0
