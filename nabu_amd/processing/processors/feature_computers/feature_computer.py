"""Base of the feature computers (reference: .../feature_computers/feature_computer.py:8-66).

The reference computes one utterance at a time with numpy; here a computer takes a list of utterances of one
sample rate and the whole list is two kernel launches (nabu_feat_compute, include/nabu_hip.h).  Host Python
only concatenates the samples and asks the library for the frame plan."""
import ctypes
from abc import ABCMeta, abstractmethod

import numpy as np

from nabu_amd import _hip
from nabu_amd.tools.default_conf import apply_defaults, defaults_path

DYNAMIC = ('nodelta', 'delta', 'ddelta')


class FeatureComputer(object, metaclass=ABCMeta):
    '''A featurecomputer is used to compute features'''
    kind = None

    def __init__(self, conf):
        '''conf: the feature configuration as a configparser; its [feature] section is merged with
        defaults/<classname>.cfg'''
        self.conf = dict(conf.items('feature'))
        apply_defaults(self.conf, defaults_path(__file__, self))
        if self.conf['dynamic'] not in DYNAMIC:
            raise Exception('unknown dynamic type: %s' % self.conf['dynamic'])
        self._tables = {}

    @abstractmethod
    def _num_static(self):
        '''static columns before the energy'''

    def get_dim(self):
        '''the feature dimension (no device is touched)'''
        dim = self._num_static() + (self.conf['include_energy'] == 'True')
        return dim * (1 + DYNAMIC.index(self.conf['dynamic']))

    def desc(self, rate, mvn=False):
        '''the nabu_feat_desc of this configuration at a sample rate'''
        c = self.conf
        return _hip.feat_desc(
            rate, self.kind, winlen=float(c['winlen']), winstep=float(c['winstep']), nfft=int(c['nfft']),
            nfilt=int(c['nfilt']), numcep=int(c.get('numcep', 0)), include_energy=c['include_energy'] == 'True',
            dynamic=c['dynamic'], mvn=mvn, lowfreq=int(c['lowfreq']), highfreq=int(c['highfreq']),
            preemph=float(c['preemph']), ceplifter=float(c.get('ceplifter', 0)))

    def num_frames(self, n_samples, rate):
        '''frames of an utterance of n_samples samples (host query of the library)'''
        n = _hip.lib().nabu_feat_num_frames(ctypes.byref(self.desc(rate)), int(n_samples))
        _hip.check(min(n, 0), 'nabu_feat_num_frames')
        return n

    def __call__(self, sig, rate):
        '''the features of one utterance as a [seq_length x feature_dim] numpy array'''
        return self.compute_batch([sig], rate)[0]

    def compute_batch(self, signals, rate, mvn=False, device=None):
        '''signals: list of 1-D int16 arrays of one sample rate -> list of [frames, dim] float32 arrays'''
        import torch
        lib = _hip.lib()
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        for sig in signals:
            if sig.dtype != np.int16 or sig.ndim != 1:
                raise _hip.NabuHipError('feature computers take 1-D int16 samples, got %s %s' % (sig.dtype, sig.shape))
        n = len(signals)
        d = self.desc(rate, mvn)
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum([len(s) for s in signals], out=offsets[1:])
        if offsets[-1] >= 2 ** 31:
            raise _hip.NabuHipError('%d samples in one batch: the offsets are int32' % offsets[-1])
        offsets = offsets.astype(np.int32)
        frame_offsets, kept = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        _hip.check(lib.nabu_feat_plan_host(ctypes.byref(d), n, offsets.ctypes.data, frame_offsets.ctypes.data,
                                           kept.ctypes.data), 'nabu_feat_plan_host')
        key = (rate, str(device))
        if key not in self._tables:
            nbytes = lib.nabu_feat_ws_bytes(ctypes.byref(d))
            host = np.zeros(nbytes, np.uint8)
            _hip.check(lib.nabu_feat_tables_host(ctypes.byref(d), host.ctypes.data, nbytes), 'nabu_feat_tables_host')
            self._tables[key] = torch.from_numpy(host).to(device)
        tables = self._tables[key]
        samples = torch.from_numpy(np.concatenate(signals)).to(device)
        plan = torch.from_numpy(np.concatenate([offsets, frame_offsets, kept])).to(device)
        dev_offsets, dev_frames, dev_kept = plan[:n + 1], plan[n + 1:2 * n + 2], plan[2 * n + 2:]
        dim = self.get_dim()
        out = torch.empty((int(frame_offsets[-1]), dim), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _hip.check(lib.nabu_feat_compute(
                ctypes.byref(d), n, int(np.diff(frame_offsets).max()), _hip.ptr(samples), dev_offsets.data_ptr(),
                dev_kept.data_ptr(), dev_frames.data_ptr(), _hip.ptr(out), _hip.ptr(tables), tables.numel(),
                _hip.stream()), 'nabu_feat_compute')
            feats = out.cpu().numpy()
        return [feats[frame_offsets[u]:frame_offsets[u + 1]] for u in range(n)]
