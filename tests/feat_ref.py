"""Host restatement of the reference's audio front end, written from the text of
nabu/processing/processors/feature_computers/{sigproc,base,fbank,mfcc}.py and audio_processor.py:49-51
(the reference itself is Python 2 / TensorFlow 1.8 and cannot be executed here).  float64 by default; every
function takes a dtype so that the same formulas can be evaluated in float32, which is what the device's error
is measured against.  The pieces scipy supplies to the reference (dct, convolve1d) are written out by hand
and pinned against scipy in tests/test_feature_processors.py."""
import math

import numpy as np

EPS = 2.0 ** -52                      # numpy.finfo(float).eps
DEFAULTS = dict(kind='fbank', winlen=0.025, winstep=0.01, nfft=512, nfilt=40, numcep=12, ceplifter=22.0,
                lowfreq=0, highfreq=-1, preemph=0.97, include_energy=True, dynamic='ddelta', mvn=True)


def py2round(x):
    """round() of Python 2: halves go away from zero (x >= 0 here)"""
    return int(math.floor(x + 0.5))


def snip_length(n, rate, winlen, winstep):
    """samples that sigproc.snip keeps of n"""
    num_frames = int((n - winlen * rate) / (winstep * rate))
    return len(range(n)[0:int(num_frames * winstep * rate + winlen * rate)])


def frame_sizes(rate, winlen, winstep):
    return py2round(winlen * rate), py2round(winstep * rate)


def num_frames(n, rate, winlen=0.025, winstep=0.01):
    """frames the front end makes of an utterance of n samples"""
    slen = snip_length(n, rate, winlen, winstep)
    frame_len, frame_step = frame_sizes(rate, winlen, winstep)
    if slen <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * slen - frame_len) / frame_step))


def preemphasis(sig, coeff, dtype=np.float64):
    sig = sig.astype(dtype)
    return np.append(sig[0], sig[1:] - dtype(coeff) * sig[:-1])


def framesig(sig, frame_len, frame_step):
    """[numframes, frame_len]; the last frame zero padded; no window"""
    slen = len(sig)
    numframes = 1 if slen <= frame_len else 1 + int(math.ceil((1.0 * slen - frame_len) / frame_step))
    padded = np.zeros((numframes - 1) * frame_step + frame_len, sig.dtype)
    padded[:slen] = sig
    idx = np.arange(frame_len)[None, :] + frame_step * np.arange(numframes)[:, None]
    return padded[idx]


def dft_direct(frames, nfft):
    """rfft(frames, nfft) as the O(n^2) sum, float64 (frames longer than nfft are refused, not cropped)"""
    frames = np.asarray(frames, np.float64)
    assert frames.shape[1] <= nfft
    n = np.arange(frames.shape[1])[:, None]
    k = np.arange(nfft // 2 + 1)[None, :]
    ang = -2.0 * np.pi * ((n * k) % nfft) / nfft
    return frames @ np.cos(ang) + 1j * (frames @ np.sin(ang))


def powspec(frames, nfft):
    assert frames.shape[1] <= nfft, 'frame_len > nfft'
    spec = np.fft.rfft(frames, nfft)
    return (spec.real ** 2 + spec.imag ** 2) / frames.dtype.type(nfft)


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.0)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def get_filterbanks(nfilt, nfft, rate, lowfreq, highfreq):
    """[nfilt, nfft/2+1] float64"""
    highfreq = highfreq if highfreq > 0 else rate // 2
    assert highfreq <= rate // 2
    melpoints = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
    bins = np.floor((nfft + 1) * mel2hz(melpoints) / rate)
    fbanks = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fbanks[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fbanks[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fbanks


def dct2_ortho_matrix(n):
    """D with dct(x, type=2, norm='ortho') = x @ D.T"""
    k = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    D = np.cos(np.pi * k * (2 * j + 1) / (2.0 * n)) * math.sqrt(2.0 / n)
    D[0] *= math.sqrt(0.5)
    return D


def lifter_weights(ncoeff, L):
    return 1 + (L / 2.0) * np.sin(np.pi * np.arange(ncoeff) / L) if L > 0 else np.ones(ncoeff)


def reflect_index(i, n):
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def deriv(x):
    """convolve1d(x, [2, 1, 0, -1, -2], axis=0) with the 'reflect' boundary:
    2 x[t+2] + x[t+1] - x[t-1] - 2 x[t-2]"""
    n = x.shape[0]
    at = lambda o: x[[reflect_index(t + o, n) for t in range(n)]]
    two = x.dtype.type(2)
    return two * (at(2) - at(-2)) + (at(1) - at(-1))


def static_features(sig, rate, conf, dtype=np.float64):
    winlen, winstep, nfft = conf['winlen'], conf['winstep'], conf['nfft']
    sig = sig[:snip_length(len(sig), rate, winlen, winstep)]
    frame_len, frame_step = frame_sizes(rate, winlen, winstep)
    frames = framesig(preemphasis(sig, conf['preemph'], dtype), frame_len, frame_step)
    pspec = powspec(frames, nfft)
    assert pspec.dtype == dtype
    eps = dtype(EPS)
    energy = np.sum(pspec, 1)
    energy = np.where(energy == 0, eps, energy)
    fb = get_filterbanks(conf['nfilt'], nfft, rate, conf['lowfreq'], conf['highfreq']).astype(dtype)
    feat = np.dot(pspec, fb.T)
    feat = np.log(np.where(feat == 0, eps, feat))
    if conf['kind'] == 'mfcc':
        D = dct2_ortho_matrix(conf['nfilt'])[:conf['numcep']].astype(dtype)
        feat = np.dot(feat, D.T) * lifter_weights(conf['numcep'], conf['ceplifter']).astype(dtype)
    if conf['include_energy']:
        feat = np.append(feat, np.log(energy)[:, None], 1)
    assert feat.dtype == dtype
    return feat


def features(sig, rate, dtype=np.float64, **overrides):
    """[frames, dim] features of int16 samples `sig`"""
    conf = dict(DEFAULTS, **overrides)
    feat = static_features(np.asarray(sig), rate, conf, dtype)
    if conf['dynamic'] == 'delta':
        feat = np.concatenate((feat, deriv(feat)), 1)
    elif conf['dynamic'] == 'ddelta':
        d = deriv(feat)
        feat = np.concatenate((feat, d, deriv(d)), 1)
    else:
        assert conf['dynamic'] == 'nodelta'
    if conf['mvn']:
        feat = (feat - np.mean(feat, 0)) / np.std(feat, 0)
    assert feat.dtype == dtype
    return feat


def speech_like(seconds, rate, seed, noise_db=-50.0, peak=12000.0):
    """Seeded int16 test signal: a harmonic series with a moving fundamental and amplitude modulation plus
    white noise `noise_db` below the peak (the floor keeps every bin above float32 rounding)."""
    rng = np.random.RandomState(seed)
    n = int(round(seconds * rate))
    t = np.arange(n) / float(rate)
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * (0.7 + 0.2 * rng.rand()) * t + rng.rand())
    phase = 2 * np.pi * np.cumsum(f0) / rate
    sig = np.zeros(n)
    for h in range(1, 20):
        if h * 170.0 < rate / 2:
            sig += np.sin(h * phase + 2 * np.pi * rng.rand()) / h
    sig *= 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + rng.rand())
    sig *= peak / max(np.abs(sig).max(), 1e-9)
    sig += rng.randn(n) * peak * 10.0 ** (noise_db / 20.0)
    return np.clip(np.round(sig), -32768, 32767).astype(np.int16)
