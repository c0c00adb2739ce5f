"""GPU tests of the audio front end (nabu_amd/csrc/features.hip) against the float64 host restatement
tests/feat_ref.py.

Tolerance: for each case e32 = max abs error of the restatement evaluated in float32 against float64 on the
same input; the device's max abs error against float64 must be at most 4 * e32 (a different summation order in
the transform and the band sums is all the device is allowed).  Independently the normalised default features
must be within 1e-3 absolute (the project's parity standard).  Every column of every frame is compared.
Each test prints its ratios (pytest -s); LABNOTES.md holds the ones measured on an MI355X."""
import gzip
import math
import os
import wave
from configparser import ConfigParser

import numpy as np
import pytest

from tests import feat_ref as R

pytestmark = pytest.mark.gpu
LOG_EPS32 = np.float32(math.log(2.0 ** -52))


def _computer(kind='fbank', **fields):
    from nabu_amd.processing.processors.feature_computers import feature_computer_factory as F
    cfg = ConfigParser()
    cfg.read_dict({'feature': dict({'feature': kind}, **{k: str(v) for k, v in fields.items()})})
    return F.factory(kind)(cfg)


def _signals(rate, seed):
    """one frame up to 10 s, the noise floor 50 dB to 30 dB below the peak"""
    frame_len = R.frame_sizes(rate, 0.025, 0.01)[0]
    secs = [frame_len / float(rate), 0.04, 0.047, 0.3, 1.0, 3.0, 10.0]
    return [R.speech_like(s, rate, seed + i, noise_db=(-50.0, -40.0, -30.0)[i % 3]) for i, s in enumerate(secs)]


CONFIGS = {
    'default': ('fbank', dict(), True),
    'static': ('fbank', dict(dynamic='nodelta', include_energy=False), False),
    'mfcc': ('mfcc', dict(), True),
    'mfcc_delta_nomvn': ('mfcc', dict(dynamic='delta'), False),
    'nfft1024': ('fbank', dict(nfft=1024, winlen=0.05), True),
}


def _max_err(a, ref):
    """max abs error over the finite entries of ref; where ref is not finite (mvn of a constant column: 0/0)
    a must be not finite too"""
    bad = ~np.isfinite(ref)
    assert np.array_equal(~np.isfinite(a), bad)
    return np.abs(np.where(bad, 0, a) - np.where(bad, 0, ref)).max()


@pytest.mark.parametrize('name,rate', [(n, r) for n in sorted(CONFIGS) for r in (8000, 16000)
                                       if (n, r) != ('nfft1024', 8000)])
def test_device_features_against_float64_restatement(name, rate):
    kind, fields, mvn = CONFIGS[name]
    if rate == 8000 and 'nfft' not in fields:
        fields = dict(fields, nfft=256)
    comp = _computer(kind, **fields)
    sigs = _signals(rate, 100 * len(name) + rate // 1000)
    if 'winlen' in fields:
        sigs = sigs[1:]
    got = comp.compute_batch(sigs, rate, mvn=mvn)
    conf = dict(fields, kind=kind, mvn=mvn)
    worst = 0.0
    for sig, dev in zip(sigs, got):
        with np.errstate(invalid='ignore', divide='ignore'):
            ref = R.features(sig, rate, **conf)
            e32 = _max_err(R.features(sig, rate, np.float32, **conf), ref)
        assert dev.shape == ref.shape and dev.dtype == np.float32
        err = _max_err(dev, ref)
        print('%s rate %d frames %d: device error %.3g, e32 %.3g, ratio %.2f' % (name, rate, ref.shape[0], err, e32,
                                                                               err / max(e32, 1e-30)))
        worst = max(worst, err / max(e32, 1e-30))
        assert err <= 4 * e32, (name, rate, ref.shape, err, e32)
        if name == 'default':
            assert err <= 1e-3
    print('%s rate %d: worst ratio %.2f' % (name, rate, worst))


@pytest.mark.parametrize('rate', [8000, 16000])
def test_short_utterances_unnormalised(rate):
    """1, 2 and 3 frames with both derivative orders (the reflection wraps more than once), mvn off"""
    comp = _computer('fbank', nfft=256 if rate == 8000 else 512)
    fl, fs = R.frame_sizes(rate, 0.025, 0.01)
    sigs = [R.speech_like((fl + k * fs) / float(rate), rate, 40 + k) for k in (0, 1, 2, 3)]
    sigs.append(R.speech_like(fl / 2.0 / rate, rate, 50))       # shorter than a frame
    got = comp.compute_batch(sigs, rate, mvn=False)
    assert [g.shape[0] for g in got] == [1, 2, 3, 4, 1]
    for sig, dev in zip(sigs, got):
        ref = R.features(sig, rate, mvn=False, nfft=comp.desc(rate).nfft)
        e32 = np.abs(R.features(sig, rate, np.float32, mvn=False, nfft=comp.desc(rate).nfft) - ref).max()
        err = np.abs(dev - ref).max()
        print('short rate %d frames %d: device error %.3g, e32 %.3g, ratio %.2f' % (rate, ref.shape[0], err, e32,
                                                                                  err / e32))
        assert err <= 4 * e32


def test_zero_frames_give_exactly_log_eps():
    comp = _computer('fbank')
    zero = np.zeros(16000, np.int16)
    holed = R.speech_like(1.0, 16000, 7)
    holed[4000:9000] = 0
    got = comp.compute_batch([zero, holed], 16000, mvn=False)
    assert got[0].shape == (98, 123)
    assert (got[0][:, :41].view(np.uint32) == LOG_EPS32.view(np.uint32)).all()
    assert (got[0][:, 41:] == 0).all()
    # frames that lie wholly inside the run of zeros (the sample before a frame enters through the pre-emphasis)
    inside = [f for f in range(98) if f * 160 - 1 >= 4000 and f * 160 + 400 <= 9000]
    assert len(inside) >= 25
    assert (got[1][inside, :41].view(np.uint32) == LOG_EPS32.view(np.uint32)).all()
    ref = R.features(holed, 16000, mvn=False)
    e32 = np.abs(R.features(holed, 16000, np.float32, mvn=False) - ref).max()
    assert np.abs(got[1] - ref).max() <= 4 * e32


def test_batch_invariance_bit_for_bit():
    comp = _computer('fbank')
    rng = np.random.RandomState(5)
    batch = [R.speech_like(float(rng.uniform(0.03, 4.0)), 16000, 200 + i) for i in range(64)]
    probe = R.speech_like(2.345, 16000, 999)
    alone = comp.compute_batch([probe], 16000, mvn=True)[0]
    for pos in (0, 31, 63):
        sigs = batch[:pos] + [probe] + batch[pos + 1:]
        assert len(sigs) == 64
        got = comp.compute_batch(sigs, 16000, mvn=True)[pos]
        assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), pos
    again = comp.compute_batch([probe], 16000, mvn=True)[0]
    assert np.array_equal(again.view(np.uint32), alone.view(np.uint32))
    mfcc = _computer('mfcc')
    a = mfcc.compute_batch([probe], 16000, mvn=True)[0]
    b = mfcc.compute_batch(batch[:20] + [probe], 16000, mvn=True)[20]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_mixed_rates_in_one_process_batch(tmp_path):
    from nabu_amd.processing.processors import processor_factory
    cfg = ConfigParser()
    cfg.read_dict({'processor': {'processor': 'audio_processor'}, 'feature': {'feature': 'fbank'}})
    proc = processor_factory.factory('audio_processor')(cfg)
    utts = [(16000, R.speech_like(1.0, 16000, 1)), (8000, R.speech_like(1.0, 8000, 2)),
            (16000, R.speech_like(0.5, 16000, 3))]
    out = proc.process_loaded(utts)
    for (rate, sig), dev in zip(utts, out):
        assert np.abs(dev - R.features(sig, rate)).max() < 1e-3


def _write_wav(path, sig, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(rate)
        w.writeframes(sig.astype('<i2').tobytes())


def test_data_script_end_to_end(tmp_path):
    from nabu_amd.scripts import data
    from nabu_amd.processing import input_pipeline
    from nabu_amd.processing.processors import processor_factory
    from nabu_amd.processing.tfreaders import tfreader_factory
    wavs = tmp_path / 'wav'
    wavs.mkdir()
    sigs = {'utt%d' % i: R.speech_like(s, 16000, 60 + i) for i, s in enumerate((1.2, 0.8, 2.0, 5.0, 0.6))}
    for name, sig in sigs.items():
        _write_wav(wavs / (name + '.wav'), sig, 16000)
    lines = {'utt0': str(wavs / 'utt0.wav'), 'utt1': 'cat %s |' % (wavs / 'utt1.wav'),
             'utt2': '%s 0.25 1.5' % (wavs / 'utt2.wav'), 'utt3': str(wavs / 'utt3.wav'),
             'utt4': 'cat %s | 0.1 0.5' % (wavs / 'utt4.wav')}
    scp = tmp_path / 'wav.scp.gz'
    with gzip.open(str(scp), 'wt') as fid:
        fid.write(''.join('%s %s\n' % kv for kv in lines.items()))
    text = tmp_path / 'text'
    text.write_text(''.join('utt%d sil aa b sil\n' % i for i in range(5)))
    fexp, texp = tmp_path / 'fexp', tmp_path / 'texp'
    fexp.mkdir(), texp.mkdir()
    fdir, tdir = str(tmp_path / 'features'), str(tmp_path / 'text_store')
    (fexp / 'database.conf').write_text('[trainfbank]\ntype = array\ndatafiles = %s\ndir = %s\n' % (scp, fdir))
    (fexp / 'processor.cfg').write_text('[processor]\nprocessor = audio_processor\nmax_length = 400\n\n'
                                        '[feature]\nfeature = fbank\n')
    (texp / 'database.conf').write_text('[traintext]\ntype = string\ndatafiles = %s\ndir = %s\n' % (text, tdir))
    (texp / 'processor.cfg').write_text('[processor]\nprocessor = text_processor\nnormalizer = phones\n'
                                        'alphabet = sil aa b\n')
    data.main(str(fexp))
    data.main(str(texp))
    # the same lines through process_batch
    cfg = ConfigParser()
    cfg.read(str(fexp / 'processor.cfg'))
    proc = processor_factory.factory('audio_processor')(cfg)
    want = dict(zip(lines, proc.process_batch(list(lines.values()))))
    assert want['utt3'] is None and want['utt2'].shape == (R.num_frames(20000, 16000), 123)      # 5 s is 498 frames > max_length
    assert np.abs(want['utt2'] - R.features(sigs['utt2'][4000:24000], 16000)).max() < 1e-3
    kept = [n for n in lines if want[n] is not None]
    scp_lines = open(os.path.join(fdir, 'pointers.scp')).read().splitlines()
    assert [l.split('\t')[0] for l in scp_lines] == kept
    reader = tfreader_factory.factory('audio_feature')([fdir])
    for line in scp_lines:
        name, path = line.split('\t')
        x, n = reader(path)
        assert n == want[name].shape[0] and np.array_equal(x, want[name])
    lens = [want[n].shape[0] for n in kept]
    assert open(os.path.join(fdir, 'max_length')).read() == str(max(lens))
    assert open(os.path.join(fdir, 'dim')).read() == '123'
    assert np.array_equal(np.load(os.path.join(fdir, 'sequence_length_histogram.npy')),
                          np.bincount(lens, minlength=max(lens) + 1))
    conf = ConfigParser()
    conf.read_dict({'trainfbank': {'type': 'audio_feature', 'dir': fdir},
                    'traintext': {'type': 'string_eos', 'dir': tdir}})
    pipe = input_pipeline.from_sections(conf, ['features'], [['trainfbank']], ['text'], [['traintext']],
                                        batch_size=2, numbuckets=1, seed=1)
    b = pipe.batch(0)
    assert b['inputs']['features'].shape[0] == 2 and b['inputs']['features'].shape[2] == 123
    assert b['targets']['text'].shape[0] == 2 and set(b['target_seq_length']['text']) == {5}
