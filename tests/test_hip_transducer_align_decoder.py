"""TransducerAlignmentDecoder and emission_times = True of TransducerDecoder on the briefly trained model of
tests/test_hip_transducer_decoder.py (trained once per session, shared): the files have the documented shape, the times
scale with frame_seconds, and the numbers are ops.transducer_align's on the model's own f and g."""
import configparser
import math

import numpy as np
import pytest
import torch

from nabu_amd import ops
from nabu_amd import variables as vs
from nabu_amd.neuralnetworks.decoders import decoder_factory
from nabu_amd.neuralnetworks.decoders.ctc_alignment_decoder import ctm_lines
from nabu_amd.neuralnetworks.decoders.transducer_alignment_decoder import emission_segments
from tests.test_hip_transducer_decoder import ALPHABET, MAX_STEPS, decoder_of, trained

pytestmark = pytest.mark.gpu
SYMBOLS = ALPHABET.split(' ')
NAMES = ['utt%d' % i for i in range(4)]


def _aligner(tr, **extra):
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': dict({'decoder': 'transducer_alignment_decoder', 'text_alphabet': ALPHABET}, **extra)})
    return decoder_factory.factory('transducer_alignment_decoder')(conf, tr.model)


def _batch(tr, data):
    batch = data.batch(0)
    return batch, tr.to_device(batch)


def _direct(tr, b):
    """ops.transducer_align on the model's own f and g for the references of the batch"""
    with torch.no_grad():
        logits, lens = tr.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)
    f, g = logits['text'].contiguous(), logits['text_pred'].contiguous()
    out = ops.transducer_align(f, g, lens['text'].dev, b['targets']['text'].to(torch.int32).contiguous(),
                               b['target_seq_length']['text'].dev)
    return [a.cpu().numpy() for a in out], lens['text'].host


def _ctm(path):
    rows = [line.split(' ') for line in open(path).read().splitlines()]
    assert all(len(r) == 6 and r[1] == '1' for r in rows)
    return rows


def test_alignment_decoder_files_and_scores(tmp_path, capsys):
    tr, data, _ = trained()
    batch, b = _batch(tr, data)
    (state, frame, conf, score, status), frames = _direct(tr, b)
    assert status[0] == 0
    ref, ref_len = batch['targets']['text'], batch['target_seq_length']['text']
    dec = _aligner(tr)
    out = dec(b['inputs'], b['input_seq_length'], targets=b['targets'], target_seq_length=b['target_seq_length'])
    assert list(out) == ['text'] and np.array_equal(out['text'][1].cpu().numpy(), frame)
    assert np.array_equal(out['text'][3].cpu().numpy().view(np.int32), score.view(np.int32))
    dec.write(out, str(tmp_path / 'frames'), NAMES)
    lines = open(str(tmp_path / 'frames' / 'text' / 'alignment')).read().splitlines()
    assert [l.split(' ')[0] for l in lines] == NAMES
    for i, line in enumerate(lines):
        cells = line.split(' ')[1:]
        assert len(cells) == frames[i]                         # one cell per ENCODED frame
        emitted = [s for c in cells if c != '_' for s in c.split('+')]
        assert emitted == [SYMBOLS[j] for j in ref[i, :ref_len[i]]]
        for t, c in enumerate(cells):
            assert (c == '_') == (not np.any(frame[i, :ref_len[i]] == t))
    scores = open(str(tmp_path / 'frames' / 'text' / 'scores')).read().splitlines()
    assert scores == ['%s %f' % (n, score[i]) for i, n in enumerate(NAMES)]
    rows = _ctm(str(tmp_path / 'frames' / 'text' / 'segments.ctm'))
    assert len(rows) == int(ref_len.sum())
    k = 0
    for i, n in enumerate(NAMES):
        starts = []
        for j in range(ref_len[i]):
            name, _, start, dur, sym, cf = rows[k]
            k += 1
            assert name == n and sym == SYMBOLS[ref[i, j]] and int(start) == frame[i, j] and int(dur) >= 1
            nxt = frame[i, j + 1] if j + 1 < ref_len[i] else frames[i]
            assert int(start) + int(dur) == max(nxt, frame[i, j] + 1)
            assert cf == '%.4f' % math.exp(float(conf[i, j])) and 0 <= float(cf) <= 1
            starts.append(int(start))
        assert starts == sorted(starts) and all(0 <= s < frames[i] for s in starts)

    # frame_seconds scales the times
    sec = _aligner(tr, frame_seconds='0.01', blank_symbol='sil')
    sec.write(sec(b['inputs'], b['input_seq_length'], targets=b['targets'], target_seq_length=b['target_seq_length']),
              str(tmp_path / 'seconds'), NAMES)
    timed = _ctm(str(tmp_path / 'seconds' / 'text' / 'segments.ctm'))
    assert len(timed) == len(rows)
    for a, c in zip(rows, timed):
        assert c[2] == '%.3f' % (int(a[2]) * 0.01) and c[3] == '%.3f' % (int(a[3]) * 0.01) and c[4:] == a[4:]
    assert ' sil' in open(str(tmp_path / 'seconds' / 'text' / 'alignment')).read()
    capsys.readouterr()

    # a reference with a label outside the alphabet: reported by name and left out; misfit = raise raises
    bad = dict(b, targets={'text': b['targets']['text'].clone()})
    bad['targets']['text'][1, 0] = len(SYMBOLS)
    out = dec(bad['inputs'], bad['input_seq_length'], targets=bad['targets'], target_seq_length=bad['target_seq_length'])
    dec.write(out, str(tmp_path / 'bad'), NAMES)
    assert 'utt1 is not aligned' in capsys.readouterr().out
    for name in ('alignment', 'scores'):
        got = [l.split(' ')[0] for l in open(str(tmp_path / 'bad' / 'text' / name)).read().splitlines()]
        assert got == ['utt0', 'utt2', 'utt3']
    assert {r[0] for r in _ctm(str(tmp_path / 'bad' / 'text' / 'segments.ctm'))} == {'utt0', 'utt2', 'utt3'}
    with pytest.raises(Exception, match='transducer: invalid utterance 1 of the batch'):
        _aligner(tr, misfit='raise')(bad['inputs'], bad['input_seq_length'], targets=bad['targets'],
                                     target_seq_length=bad['target_seq_length'])


@pytest.mark.parametrize('width', [None, 4])
def test_emission_times_of_the_recognised_labels(tmp_path, width):
    tr, data, _ = trained()
    batch, b = _batch(tr, data)
    extra = {} if width is None else {'beam_width': str(width)}
    plain = decoder_of(tr, **extra)
    ids0, lens0 = plain(b['inputs'], b['input_seq_length'])['text']
    dec = decoder_of(tr, emission_times='True', frame_seconds='0.02', **extra)
    out = dec(b['inputs'], b['input_seq_length'])['text']
    ids, lens, seg, conf, score = out
    assert torch.equal(ids, ids0) and torch.equal(lens, lens0) and int(lens.max()) >= 2
    assert tuple(seg.shape) == (4, MAX_STEPS, 2) and tuple(conf.shape) == (4, MAX_STEPS)

    # the same through a direct call: f from the model, g teacher-forced on the recognised ids
    with torch.no_grad():
        logits, flen = tr.model(b['inputs'], b['input_seq_length'], targets=[], target_seq_length=[], is_training=False)
        L = int(lens.max())
        labels = ids[:, :L].clamp(min=0).contiguous()
        with vs.as_default(tr.model.store):
            g = tr.model.decoder.predict_sequence('text', labels, lens)
        # (the model's own teacher-forced pass gives the same g)
        both, _ = tr.model(b['inputs'], b['input_seq_length'], {'text': labels}, {'text': lens}, False)
        assert torch.equal(both['text_pred'], g)
    f = logits['text'].contiguous()
    enc = flen['text'].dev if hasattr(flen['text'], 'dev') else flen['text']
    _, frame, cf, sc, status = ops.transducer_align(f, g, enc, labels, lens)
    assert int(status.item()) == 0
    assert torch.equal(score, sc) and torch.equal(conf[:, :L], cf) and bool((conf[:, L:] == 0).all())
    want = emission_segments(frame, lens, enc)
    assert torch.equal(seg[:, :L], want) and bool((seg[:, L:] == -1).all())

    dec.write({'text': out}, str(tmp_path), NAMES)
    ids_h, lens_h = ids.cpu().numpy(), lens.cpu().numpy()
    text = open(str(tmp_path / 'text')).read().splitlines()
    assert text == ['%s %s' % (n, ' '.join(SYMBOLS[j] for j in ids_h[i, :lens_h[i]])) for i, n in enumerate(NAMES)]
    expect = []
    for i, n in enumerate(NAMES):
        expect += ctm_lines(n, want[i, :lens_h[i]].cpu().numpy(), cf[i, :lens_h[i]].cpu().numpy(),
                            [SYMBOLS[j] for j in ids_h[i, :lens_h[i]]], 0.02)
    assert open(str(tmp_path / 'text.ctm')).read() == ''.join(expect) and len(expect) == int(lens_h.sum())
    fr = frame.cpu().numpy()
    for i in range(4):
        assert np.all(np.diff(fr[i, :lens_h[i]]) >= 0) and np.all(fr[i, :lens_h[i]] < int(enc[i]))
