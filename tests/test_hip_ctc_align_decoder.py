"""CTCAlignmentDecoder, the Recognizer's references and the CTC decoder's time stamps on the GPU, on tiny models."""
import configparser
import os

import numpy as np
import pytest
import torch

from nabu_amd import ops, recipes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SYMBOLS = ['s%d' % i for i in range(39)]
ALPHABET = ' '.join(SYMBOLS)


def conf_of(decoder, **keys):
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': decoder}, **keys)})
    return conf


def ctc_model(**overrides):
    from nabu_amd.neuralnetworks.models.model import Model
    mc, tc, _ = recipes.load_recipe('cfg1_dblstm_ctc', **dict({'encoder.num_units': 16, 'encoder.num_layers': 2}, **overrides))
    return Model(mc, int(tc.get('trainer', 'trainlabels')), None, seed=4)


def las_model(**overrides):
    from nabu_amd.neuralnetworks.models.model import Model
    mc, tc, _ = recipes.load_recipe('cfg3_las_vanilla', **dict({'encoder.num_units': 16, 'decoder.num_units': 16}, **overrides))
    return Model(mc, int(tc.get('trainer', 'trainlabels')), None, seed=4)


def collapse(symbols, blank='_'):
    out, prev = [], None
    for s in symbols:
        if s != prev and s != blank:
            out.append(s)
        prev = s
    return out


def read_lines(path):
    with open(path) as fid:
        return [line.split() for line in fid.read().splitlines()]


def check_files(directory, output, names, texts, frames, frame_seconds=0.0):
    """all three files; every alignment line collapses to its text; the ctm segments tile its non-blank frames"""
    align = {r[0]: r[1:] for r in read_lines(os.path.join(directory, output, 'alignment'))}
    scores = {r[0]: float(r[1]) for r in read_lines(os.path.join(directory, output, 'scores'))}
    ctm = {}
    for r in read_lines(os.path.join(directory, output, 'segments.ctm')):
        assert len(r) == 6 and r[1] == '1'
        ctm.setdefault(r[0], []).append(r[2:])
    assert sorted(align) == sorted(names) == sorted(scores)
    for name in names:
        line = align[name]
        assert len(line) == frames[name], (name, len(line), frames[name])
        assert collapse(line) == texts[name], (name, line, texts[name])
        assert np.isfinite(scores[name]) and scores[name] < 0
        covered, segs = [], ctm.get(name, [])
        assert [s[2] for s in segs] == texts[name]
        for start, dur, sym, cf in segs:
            if frame_seconds > 0:
                a, n = float(start) / frame_seconds, float(dur) / frame_seconds
                assert abs(a - round(a)) < 0.02 and abs(n - round(n)) < 0.02, (start, dur)
                a, n = int(round(a)), int(round(n))
            else:
                a, n = int(start), int(dur)
            assert n >= 1 and all(line[t] == sym for t in range(a, a + n))
            assert 0.0 < float(cf) <= 1.0
            covered += list(range(a, a + n))
        assert covered == [t for t, s in enumerate(line) if s != '_'], name


def synthetic_batch(eos, time_reduction, max_labels):
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(3, 64 if eos else 30, 40, min_frames=48 if eos else 22, min_labels=1, max_labels=max_labels,
                         eos=eos, time_reduction=time_reduction, seed=31)
    b = data.batch(0)
    x = torch.tensor(b['inputs']['features'], device=DEV)
    il = SeqLen(b['input_seq_length']['features'], DEV)
    return b, x, il


def test_alignment_decoder_on_a_ctc_model(tmp_path):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    model = ctc_model()
    b, x, il = synthetic_batch(False, 1, 5)
    tg, tl = b['targets']['text'], b['target_seq_length']['text']
    names = ['u0', 'u1', 'u2']
    texts = {n: [SYMBOLS[j] for j in tg[i, :tl[i]]] for i, n in enumerate(names)}
    frames = {n: int(b['input_seq_length']['features'][i]) for i, n in enumerate(names)}
    cls = decoder_factory.factory('ctc_alignment_decoder')
    assert cls.needs_targets
    for k, fs in enumerate((0.0, 0.04)):
        dec = cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET, frame_seconds=str(fs)), model)
        out = dec({'features': x}, {'features': il}, targets={'text': torch.tensor(tg, device=DEV)},
                  target_seq_length={'text': tl})
        d = str(tmp_path / ('d%d' % k))
        os.makedirs(d)
        dec.write(out, d, names)
        check_files(d, 'text', names, texts, frames, fs)
        with pytest.raises(Exception, match='validate'):
            dec.update_evaluation_loss([0.0], out, None, None)
    # the same numbers in both files: seconds = frames * 0.04
    f0 = read_lines(str(tmp_path / 'd0' / 'text' / 'segments.ctm'))
    f1 = read_lines(str(tmp_path / 'd1' / 'text' / 'segments.ctm'))
    for r0, r1 in zip(f0, f1):
        assert r1[2] == '%.3f' % (int(r0[2]) * 0.04) and r1[3] == '%.3f' % (int(r0[3]) * 0.04)
    # an utterance that does not fit: reported by name, in none of the files, the others written
    tl2 = tl.copy()
    tg2 = np.zeros((3, 40), np.int32)
    tg2[:, :tg.shape[1]] = tg
    tg2[1] = np.arange(40) % 7
    tl2[1] = 40
    out = dec({'features': x}, {'features': il}, targets={'text': torch.tensor(tg2, device=DEV)},
              target_seq_length={'text': tl2})
    d = str(tmp_path / 'misfit')
    os.makedirs(d)
    dec.write(out, d, names)
    for f in ('alignment', 'segments.ctm', 'scores'):
        assert {r[0] for r in read_lines(os.path.join(d, 'text', f))} == {'u0', 'u2'}
    strict = cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET, misfit='raise'), model)
    with pytest.raises(Exception, match='Not enough time'):
        strict({'features': x}, {'features': il}, targets={'text': torch.tensor(tg2, device=DEV)},
               target_seq_length={'text': tl2})


def test_alignment_decoder_on_a_speller_with_a_ctc_head(tmp_path):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    model = las_model(**{'decoder.ctc_head': 'True'})
    b, x, il = synthetic_batch(True, 8, 3)
    tg, tl = b['targets']['text'], b['target_seq_length']['text']
    names = ['u0', 'u1', 'u2']
    texts = {n: [SYMBOLS[j] for j in tg[i, :tl[i] - 1]] for i, n in enumerate(names)}      # without the end label
    frames = {n: -(-int(b['input_seq_length']['features'][i]) // 8) for i, n in enumerate(names)}
    dec = decoder_factory.factory('ctc_alignment_decoder')(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET), model)
    out = dec({'features': x}, {'features': il}, targets={'text': torch.tensor(tg, device=DEV)},
              target_seq_length={'text': tl})
    assert [int(n) for n in out['text'][4]] == [frames[n] for n in names]
    dec.write(out, str(tmp_path), names)
    check_files(str(tmp_path), 'text', names, texts, frames)


def test_refusals_at_construction():
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    from nabu_amd.neuralnetworks.models.model import Model
    cls = decoder_factory.factory('ctc_alignment_decoder')
    with pytest.raises(ValueError, match='CTC head'):
        cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET), las_model())
    mc, _, _ = recipes.load_recipe('dnn_hybrid_wsj', **{'encoder.num_units': 16, 'encoder.num_layers': 2})
    with pytest.raises(ValueError, match='dnn encoder'):
        cls(conf_of('ctc_alignment_decoder', alignments_alphabet='a b'), Model(mc, 0, None, seed=1))
    with pytest.raises(ValueError, match='lm_file'):
        cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET, lm_file='x.npz'), ctc_model())
    with pytest.raises(ValueError, match='ctc_weight'):
        cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET, ctc_weight='0.3'), ctc_model())
    with pytest.raises(ValueError, match='frame_seconds'):
        cls(conf_of('ctc_alignment_decoder', text_alphabet=ALPHABET, frame_seconds='-1'), ctc_model())


def test_recognizer_passes_the_references(tmp_path):
    from nabu_amd.neuralnetworks.recognizer import Recognizer
    from tests.test_data_path import make_dataset
    dataconf, feats, texts, alphabet = make_dataset(str(tmp_path / 'data'), n=7, dim=40, seed=2, min_frames=20)
    model = ctc_model(**{'io.output_dims': '4'})
    conf = conf_of('ctc_alignment_decoder', text_alphabet=' '.join(alphabet))
    conf.read_dict({'recognizer': {'batch_size': '3', 'features': 'trainfbank'}})
    with pytest.raises(ValueError, match='text'):
        Recognizer(model, conf, dataconf, str(tmp_path))         # no target key
    conf.set('recognizer', 'text', 'traintext')
    rec = Recognizer(model, conf, dataconf, str(tmp_path))
    assert rec.numbatches == 3
    directory = rec.recognize()
    names = sorted(feats)
    check_files(directory, 'text', names, {n: texts[n].split() for n in names}, {n: feats[n].shape[0] for n in names})
    # a decoder without the attribute is built and fed as ever: no target sections are read
    plain = conf_of('ctc_decoder', text_alphabet=' '.join(alphabet))
    plain.read_dict({'recognizer': {'batch_size': '3', 'features': 'trainfbank'}})
    rec = Recognizer(model, plain, dataconf, str(tmp_path))
    assert rec.target_names == [] and rec.data.target_names == []


def test_ctc_decoder_time_stamps(tmp_path):
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    model = ctc_model()
    b, x, il = synthetic_batch(False, 1, 5)
    names = ['u0', 'u1', 'u2']
    cls = decoder_factory.factory('ctc_decoder')
    plain = cls(conf_of('ctc_decoder', text_alphabet=ALPHABET), model)
    stamped = cls(conf_of('ctc_decoder', text_alphabet=ALPHABET, timestamps='True'), model)
    d0, d1 = str(tmp_path / 'plain'), str(tmp_path / 'stamped')
    os.makedirs(d0)
    os.makedirs(d1)
    out0 = plain({'features': x}, {'features': il})
    assert len(out0['text']) == 2
    plain.write(out0, d0, names)
    # without the key: the file the search's own result gives, byte for byte, and nothing else
    with torch.no_grad():
        logits, ll = model({'features': x}, {'features': il}, [], [], False)
    ids, lens, _ = ops.ctc_beam_search(logits['text'], ll['text'].dev, 100, merge_repeated=True)
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    want = ''.join('%s %s\n' % (n, ' '.join(SYMBOLS[j] for j in ids[i, :lens[i]])) for i, n in enumerate(names))
    assert open(os.path.join(d0, 'text')).read() == want
    assert os.listdir(d0) == ['text']
    out1 = stamped({'features': x}, {'features': il})
    assert len(out1['text']) == 5 and torch.equal(out1['text'][0], out0['text'][0])
    stamped.write(out1, d1, names)
    assert open(os.path.join(d1, 'text')).read() == want and sorted(os.listdir(d1)) == ['text', 'text.ctm']
    ctm = {}
    for r in read_lines(os.path.join(d1, 'text.ctm')):
        assert len(r) == 6 and r[1] == '1' and int(r[3]) >= 1 and 0.0 < float(r[5]) <= 1.0
        ctm.setdefault(r[0], []).append(r)
    for i, n in enumerate(names):
        rows = ctm.get(n, [])
        assert [r[4] for r in rows] == [SYMBOLS[j] for j in ids[i, :lens[i]]]
        ends = [int(r[2]) + int(r[3]) for r in rows]
        assert all(int(r[2]) >= e for r, e in zip(rows[1:], ends)) and all(e <= int(il.host[i]) for e in ends)
    loss = [0.0]
    stamped.update_evaluation_loss(loss, out1, {'text': b['targets']['text']}, {'text': b['target_seq_length']['text']})
    assert np.isfinite(loss[0])
