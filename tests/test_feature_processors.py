"""CPU tests of the audio front end: the host restatement tests/feat_ref.py is pinned (against scipy where it
is installed, closed-form cases, a committed fixture), and the host side of the feature ABI, the processors
package and the cfg defaults are checked against it.  No GPU is needed."""
import ctypes
import gzip
import math
import os
import sys
import wave
from configparser import ConfigParser

import numpy as np
import pytest

from tests import feat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_EPS = math.log(2.0 ** -52)


# ---------------------------------------------------------------- the restatement itself
def test_direct_dft_dct_and_reflect_convolution_match_scipy():
    fft = pytest.importorskip('scipy.fft')
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(0)
    frames = rng.randn(5, 400)
    want = fft.rfft(frames, 512)
    assert np.abs(R.dft_direct(frames, 512) - want).max() < 1e-10
    assert np.abs(R.powspec(frames, 512) - np.abs(want) ** 2 / 512).max() < 1e-9
    x = rng.randn(7, 40)
    assert np.abs(x @ R.dct2_ortho_matrix(40).T - fft.dct(x, type=2, axis=1, norm='ortho')).max() < 1e-12
    for n in (1, 2, 3, 4, 5, 9, 50):
        x = rng.randn(n, 3)
        assert np.abs(R.deriv(x) - ndimage.convolve1d(x, [2, 1, 0, -1, -2], 0)).max() < 1e-12, n


def test_fft_path_equals_direct_dft_without_scipy():
    frames = np.random.RandomState(1).randn(4, 400)
    direct = R.dft_direct(frames, 512)
    assert np.abs(R.powspec(frames, 512) - (direct.real ** 2 + direct.imag ** 2) / 512).max() < 1e-9


def test_derivatives_of_one_two_and_three_frames_by_hand():
    a, b, c = 1.0, 10.0, 100.0
    # one frame: every neighbour is the frame itself
    assert R.deriv(np.array([[a]])).tolist() == [[0.0]]
    # a b  ->  extended  b a | a b | b a
    #   t=0: 2 x[2] + x[1] - x[-1] - 2 x[-2] = 2b + b - a - 2b ; t=1: 2 x[3] + x[2] - x[0] - 2 x[-1] = 2a + b - a - 2a
    assert R.deriv(np.array([[a], [b]])).ravel().tolist() == [2 * b + b - a - 2 * b, 2 * a + b - a - 2 * a]
    # a b c  ->  c b a | a b c | c b a
    want = [2 * c + b - a - 2 * b, 2 * c + c - a - 2 * a, 2 * b + c - b - 2 * a]
    assert R.deriv(np.array([[a], [b], [c]])).ravel().tolist() == want


def test_zero_and_constant_signals():
    zero = np.zeros(16000, np.int16)
    feat = R.features(zero, 16000, mvn=False)
    assert feat.shape == (98, 123)
    assert (feat[:, :41] == LOG_EPS).all() and (feat[:, 41:] == 0).all()
    # 1 s at 16 kHz: int((16000 - 400) / 160) = 97 -> 15920 samples -> 1 + ceil(15520 / 160) = 98 frames
    const = np.full(16000, 1000, np.int16)
    assert R.features(const, 16000, mvn=False).shape[0] == 98 == R.num_frames(16000, 16000)
    assert R.num_frames(399, 16000) == R.num_frames(400, 16000) == R.num_frames(559, 16000) == 1
    assert R.num_frames(560, 16000) == 2
    assert R.frame_sizes(22050, 0.025, 0.01) == (551, 221)         # 551.25 -> 551, 220.5 -> 221 (Python 3: 220)
    assert R.frame_sizes(44100, 0.025, 0.01) == (1103, 441)        # 1102.5 -> 1103 (Python 3: 1102)
    with pytest.raises(AssertionError):                            # numpy would crop the frame to nfft
        R.features(const, 44100, nfft=1024)


def test_float32_evaluation_stays_close_to_float64():
    sig = R.speech_like(1.0, 16000, 5)
    assert np.abs(R.features(sig, 16000, np.float32) - R.features(sig, 16000)).max() < 1e-3


def test_committed_fixture_pins_the_restatement():
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    try:
        import make_features_golden as G
    finally:
        sys.path.pop(0)
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'features.npz')) as z:
        for name, (rate, seconds, seed, conf) in G.CASES.items():
            sig = z[name + '.signal']
            assert sig.dtype == np.int16 and np.array_equal(sig, R.speech_like(seconds, rate, seed)), name
            got = R.features(sig, rate, **conf)
            assert got.shape == z[name + '.features'].shape
            assert np.abs(got - z[name + '.features']).max() < 1e-8, name


# ---------------------------------------------------------------- host side of the C ABI
def _lib():
    from nabu_amd import build, _hip
    build.build(verbose=False)
    return _hip, _hip.lib()


@pytest.mark.parametrize('rate,nfft', [(8000, 256), (16000, 512), (22050, 1024), (44100, 2048)])
def test_frame_count_query_equals_the_restatement(rate, nfft):
    _hip, lib = _lib()
    d = _hip.feat_desc(rate, nfft=nfft)
    frame_len, frame_step = R.frame_sizes(rate, 0.025, 0.01)
    assert (d.frame_len, d.frame_step) == (frame_len, frame_step)
    lengths = set(range(1, 40)) | {rate, 3 * rate + 7, 10 * rate}
    for centre in (frame_len, frame_len + frame_step, frame_len + 2 * frame_step, 50 * frame_step, rate):
        lengths |= set(range(max(1, centre - 3), centre + 4))
    for n in sorted(lengths):
        assert lib.nabu_feat_num_frames(ctypes.byref(d), n) == R.num_frames(n, rate), (rate, n)
    # the batch plan agrees with the single query and keeps what the snip keeps
    lens = sorted(lengths)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    frames, kept = np.zeros(len(lens) + 1, np.int32), np.zeros(len(lens), np.int32)
    assert lib.nabu_feat_plan_host(ctypes.byref(d), len(lens), offs.ctypes.data, frames.ctypes.data,
                                   kept.ctypes.data) == 0
    assert np.diff(frames).tolist() == [R.num_frames(n, rate) for n in lens]
    assert kept.tolist() == [R.snip_length(n, rate, 0.025, 0.01) for n in lens]


def test_bad_feature_descriptors_are_rejected_with_a_message():
    _hip, lib = _lib()
    ok = _hip.feat_desc(16000)
    assert lib.nabu_feat_dim(ctypes.byref(ok)) == 123 and lib.nabu_feat_ws_bytes(ctypes.byref(ok)) > 0
    d = _hip.feat_desc(16000, nfft=500)
    assert lib.nabu_feat_num_frames(ctypes.byref(d), 16000) == -2 and b'power of two' in lib.nabu_last_error()
    assert lib.nabu_feat_ws_bytes(ctypes.byref(d)) == 0
    d = _hip.feat_desc(44100, nfft=1024)                     # 1103 samples per frame
    assert lib.nabu_feat_num_frames(ctypes.byref(d), 44100) == -2 and b'cropped' in lib.nabu_last_error()
    for field, value, word in (('size', 8, b'size'), ('frame_step', 161, b'round'), ('frame_len', 0, b'round'),
                               ('dynamic', 3, b'dynamic'), ('kind', 2, b'kind'), ('nfilt', 0, b'nfilt'),
                               ('highfreq', 9000, b'highfreq'), ('rate', 0, b'rate'), ('mvn', 2, b'mvn')):
        d = _hip.feat_desc(16000)
        setattr(d, field, value)
        assert lib.nabu_feat_num_frames(ctypes.byref(d), 16000) == -1, field
        assert word in lib.nabu_last_error(), (field, lib.nabu_last_error())
    d = _hip.feat_desc(16000, 'mfcc', numcep=41)
    assert lib.nabu_feat_dim(ctypes.byref(d)) == -1 and b'numcep' in lib.nabu_last_error()
    assert lib.nabu_feat_num_frames(ctypes.byref(ok), 0) == -1
    one = ctypes.c_void_p(256)
    assert lib.nabu_feat_compute(ctypes.byref(ok), 1, 1, None, one, one, one, one, one, 1 << 20, None) == -1
    assert lib.nabu_feat_compute(ctypes.byref(ok), 1, 1, one, one, one, one, one, one, 16, None) == -3
    assert lib.nabu_feat_tables_host(ctypes.byref(ok), one, 16) == -3


def test_host_tables_equal_the_restatement():
    _hip, lib = _lib()
    d = _hip.feat_desc(16000, 'mfcc')
    nbytes = lib.nabu_feat_ws_bytes(ctypes.byref(d))
    host = np.zeros(nbytes, np.uint8)
    assert lib.nabu_feat_tables_host(ctypes.byref(d), host.ctypes.data, nbytes) == 0
    tw = host[:2048].view(np.float32).reshape(256, 2)
    ang = -2 * np.pi * np.arange(256) / 512
    assert np.abs(tw[:, 0] - np.cos(ang)).max() < 1e-7 and np.abs(tw[:, 1] - np.sin(ang)).max() < 1e-7
    band = host[2048:2048 + 480].view(np.int32).reshape(3, 40)
    weights = host[2048 + 480:].view(np.float32)
    dense = np.zeros((40, 257))
    for j in range(40):
        start, length, off = band[:, j]
        dense[j, start:start + length] = weights[off:off + length]
    assert np.abs(dense - R.get_filterbanks(40, 512, 16000, 0, -1)).max() < 1e-7


# ---------------------------------------------------------------- cfg defaults, factories, processors
def _cfg(feature='fbank', processor=None, **fields):
    cfg = ConfigParser()
    cfg.read_dict({'processor': dict({'processor': 'audio_processor'}, **(processor or {})),
                   'feature': dict({'feature': feature}, **fields)})
    return cfg


@pytest.mark.parametrize('feature,static', [('fbank', 40), ('mfcc', 12)])
def test_defaults_and_get_dim(feature, static):
    from nabu_amd.processing.processors.feature_computers import feature_computer_factory as F
    for energy in ('True', 'False'):
        for order, dynamic in enumerate(('nodelta', 'delta', 'ddelta')):
            comp = F.factory(feature)(_cfg(feature, dynamic=dynamic, include_energy=energy))
            assert comp.get_dim() == (static + (energy == 'True')) * (order + 1)
    comp = F.factory(feature)(_cfg(feature))
    assert comp.conf['winlen'] == '0.025' and comp.conf['preemph'] == '0.97' and comp.conf['dynamic'] == 'ddelta'
    assert int(comp.conf['highfreq']) < 0                      # absent highfreq: half the sample rate
    d = comp.desc(16000)
    assert (d.frame_len, d.frame_step, d.nfft, d.nfilt, d.highfreq) == (400, 160, 512, 40, -1)
    assert comp.num_frames(16000, 16000) == 98
    with pytest.raises(Exception, match='Undefined feature type'):
        F.factory('ssc_like')
    with pytest.raises(Exception, match='unknown dynamic'):
        F.factory(feature)(_cfg(feature, dynamic='dddelta'))


def test_factories_raise_on_unknown_names():
    from nabu_amd.processing.processors import processor_factory
    from nabu_amd.processing.target_normalizers import normalizer_factory
    with pytest.raises(Exception, match='unknown processor type'):
        processor_factory.factory('video_processor')
    with pytest.raises(Exception, match='outside'):
        processor_factory.factory('binary_processor')
    with pytest.raises(Exception, match='Undefined normalizer'):
        normalizer_factory.factory('latin')
    assert normalizer_factory.factory('phones')('sil aa b', ['sil']) == 'sil aa b'


SHIPPED = {      # the [processor] / [feature] fields of the reference's four feature_processor.cfg files
    'DBLSTM/TIMIT': ('audio_processor', 'fbank'), 'LAS/TIMIT': ('audio_processor', 'fbank'),
    'LAS/GP': ('audio_processor', 'fbank'), 'DNN/WSJ': ('audio_processor', 'fbank'),
}


@pytest.mark.parametrize('recipe', sorted(SHIPPED))
def test_shipped_feature_processor_cfgs_build_an_audio_processor(recipe, tmp_path):
    from nabu_amd.processing.processors import processor_factory
    processor, feature = SHIPPED[recipe]
    path = tmp_path / 'feature_processor.cfg'
    path.write_text('[processor]\n#type of processor\nprocessor = %s\n\n[feature]\n#feature type\nfeature = %s\n'
                    % (processor, feature))
    cfg = ConfigParser()
    cfg.read(str(path))
    proc = processor_factory.factory(cfg.get('processor', 'processor'))(cfg)
    assert proc.get_dim() == proc.dim == 123 and proc.conf['mvn'] == 'True' and proc.conf['max_length'] == 'None'


def _write_wav(path, sig, rate, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels), w.setsampwidth(width), w.setframerate(rate)
        w.writeframes(sig.astype('<i2').tobytes() if width == 2 else sig.astype(np.uint8).tobytes())


def test_wav_path_pipe_and_segment_lines(tmp_path):
    from nabu_amd.processing.processors.audio_processor import read_wav
    sig = R.speech_like(0.5, 16000, 3)
    path = tmp_path / 'utt one.wav'                            # a space in the path: segments split from the right
    _write_wav(path, sig, 16000)
    rate, got = read_wav(str(path))
    assert rate == 16000 and got.dtype == np.int16 and np.array_equal(got, sig)
    rate, got = read_wav('cat "%s" |' % path)
    assert rate == 16000 and np.array_equal(got, sig)
    rate, got = read_wav('%s 0.1 0.35' % path)
    assert np.array_equal(got, sig[1600:5600])
    rate, got = read_wav('cat "%s" | 0.1 0.35' % path)
    assert np.array_equal(got, sig[1600:5600])
    stereo = tmp_path / 'stereo.wav'
    _write_wav(stereo, np.repeat(sig, 2), 16000, channels=2)
    with pytest.raises(Exception, match='stereo.wav.*mono 16-bit'):
        read_wav(str(stereo))
    bytes8 = tmp_path / 'eight.wav'
    _write_wav(bytes8, np.arange(100), 8000, width=1)
    with pytest.raises(Exception, match='eight.wav'):
        read_wav(str(bytes8))
    junk = tmp_path / 'junk.wav'
    junk.write_bytes(b'not a wav file at all')
    with pytest.raises(Exception, match='junk.wav'):
        read_wav(str(junk))
    with pytest.raises(Exception, match='neither a file'):
        read_wav(str(tmp_path / 'missing.wav'))


def test_max_length_drops_and_metadata_files(tmp_path, monkeypatch):
    """the bookkeeping of AudioProcessor around the device call (which is replaced by a stand-in of the right
    shapes: the device path itself is tests/test_hip_features.py)"""
    from nabu_amd.processing.processors import processor_factory
    from nabu_amd.processing.processors.feature_computers import feature_computer
    proc = processor_factory.factory('audio_processor')(_cfg(processor={'max_length': '60'}))

    def stand_in(self, signals, rate, mvn=False, device=None):
        assert mvn is True
        return [np.zeros((self.num_frames(len(s), rate), self.get_dim()), np.float32) for s in signals]
    monkeypatch.setattr(feature_computer.FeatureComputer, 'compute_batch', stand_in)
    utts = [(16000, np.zeros(n, np.int16)) for n in (8000, 16000, 400, 9840, 8000)]     # 48, 98, 1, 60, 48 frames
    out = proc.process_loaded(utts)
    assert [None if o is None else o.shape[0] for o in out] == [48, None, 1, 60, 48]
    assert proc.max_length == 60
    hist = np.zeros(61, np.int32)
    hist[[1, 60]] = 1
    hist[48] = 2
    assert np.array_equal(proc.sequence_length_histogram, hist)
    datadir = tmp_path / 'features'
    datadir.mkdir()
    proc.write_metadata(str(datadir))
    assert (datadir / 'max_length').read_text() == '60' and (datadir / 'dim').read_text() == '123'
    assert np.array_equal(np.load(str(datadir / 'sequence_length_histogram.npy')), hist)
    # what audio_feature_reader reads
    from nabu_amd.processing.tfreaders import audio_feature_reader     # noqa: F401


def test_text_processor_and_data_script_on_a_text_section(tmp_path):
    """run data on a string section: no device involved"""
    from nabu_amd.scripts import data
    expdir = tmp_path / 'exp'
    expdir.mkdir()
    text = tmp_path / 'text.gz'
    with gzip.open(str(text), 'wt') as fid:
        fid.write('utt1 sil aa b sil\nutt2 sil b sil\nutt3 sil aa aa aa b sil\n')
    (expdir / 'database.conf').write_text('[traintext]\ntype = string\ndatafiles = %s\ndir = %s\n'
                                          % (text, tmp_path / 'store'))
    (expdir / 'processor.cfg').write_text('[processor]\nprocessor = text_processor\nnormalizer = phones\n'
                                          'alphabet = sil aa b\nmax_length = 5\n')
    data.main(str(expdir))
    store = tmp_path / 'store'
    assert (store / 'max_length').read_text() == '4' and (store / 'dim').read_text() == '3'
    assert (store / 'alphabet').read_text() == 'sil aa b' and (store / 'nonesymbol').read_text() == ''
    assert np.load(str(store / 'sequence_length_histogram.npy')).tolist() == [0, 0, 0, 1, 1]
    names = [l.split('\t')[0] for l in (store / 'pointers.scp').read_text().splitlines()]
    assert names == ['utt1', 'utt2']
    from nabu_amd.processing import tfrecord
    path = (store / 'pointers.scp').read_text().splitlines()[0].split('\t')[1]
    assert b'sil aa b sil' in open(path, 'rb').read()
    assert tfrecord is not None
