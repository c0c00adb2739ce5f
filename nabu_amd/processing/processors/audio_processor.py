"""AudioProcessor (reference: nabu/processing/processors/audio_processor.py:13-125): reads audio, computes
features on the device and keeps the metadata audio_feature_reader needs.

A data line is a path to a wav file, a shell command ending in '|' whose output is a wav file, or either of
them followed by ` begin end` (seconds) for a segment.  Audio is read with the standard library's `wave`:
mono 16-bit PCM."""
import io
import os
import subprocess
import wave

import numpy as np

from nabu_amd.processing.processors import processor
from nabu_amd.processing.processors.feature_computers import feature_computer_factory


class AudioProcessor(processor.Processor):
    '''a processor for audio files, this will compute features'''

    def __init__(self, conf):
        self.comp = feature_computer_factory.factory(conf.get('feature', 'feature'))(conf)
        self.dim = self.comp.get_dim()
        self.max_length = 0
        self.sequence_length_histogram = np.zeros(0, dtype=np.int32)
        super(AudioProcessor, self).__init__(conf)

    def get_dim(self):
        return self.dim

    def __call__(self, dataline):
        '''the features of one data line as a numpy array, None when it has more than max_length frames'''
        return self.process_batch([dataline])[0]

    @staticmethod
    def load(dataline):
        '''(sample rate, int16 samples) of a data line'''
        return read_wav(dataline)

    def process_batch(self, datalines):
        '''the features of every data line in one pass over the device (None where dropped)'''
        return self.process_loaded([read_wav(line) for line in datalines])

    def process_loaded(self, utterances):
        '''utterances: list of (rate, int16 samples) as read_wav returns them.  Utterances of one sample rate
        share a device call; the result keeps the order of the input.'''
        mvn = self.conf['mvn'] == 'True'
        results = [None] * len(utterances)
        for rate in sorted(set(r for r, _ in utterances)):
            idx = [i for i, (r, _) in enumerate(utterances) if r == rate]
            for i, feat in zip(idx, self.comp.compute_batch([utterances[i][1] for i in idx], rate, mvn=mvn)):
                results[i] = feat
        max_length = self._max_length()
        for i, feat in enumerate(results):
            if max_length and feat.shape[0] > max_length:
                results[i] = None
            else:
                self._count(feat.shape[0])
        return results

    def write_metadata(self, datadir):
        with open(os.path.join(datadir, 'sequence_length_histogram.npy'), 'wb') as fid:
            np.save(fid, self.sequence_length_histogram)
        with open(os.path.join(datadir, 'max_length'), 'w') as fid:
            fid.write(str(self.max_length))
        with open(os.path.join(datadir, 'dim'), 'w') as fid:
            fid.write(str(self.dim))


def _decode(fid, name):
    try:
        with wave.open(fid, 'rb') as wav:
            if wav.getnchannels() != 1 or wav.getsampwidth() != 2 or wav.getcomptype() != 'NONE':
                raise Exception('%s: %d channel(s) of %d-bit %s audio; only mono 16-bit PCM is read'
                                % (name, wav.getnchannels(), 8 * wav.getsampwidth(), wav.getcomptype()))
            return wav.getframerate(), np.frombuffer(wav.readframes(wav.getnframes()), '<i2').astype(np.int16)
    except (wave.Error, EOFError) as err:
        raise Exception('%s: not a PCM wav file (%s)' % (name, err))


def read_wav(dataline):
    '''(sample rate, int16 samples) of a data line'''
    if os.path.exists(dataline):
        with open(dataline, 'rb') as fid:
            return _decode(fid, dataline)
    if dataline.endswith('|'):
        done = subprocess.run(dataline[:-1], shell=True, stdout=subprocess.PIPE)
        if done.returncode != 0:
            raise Exception('%s: the command failed with status %d' % (dataline, done.returncode))
        return _decode(io.BytesIO(done.stdout), dataline)
    split = dataline.split(' ')
    if len(split) < 3:
        raise Exception('%s: neither a file, a command ending in |, nor a segment of one' % dataline)
    begin, end = float(split[-2]), float(split[-1])
    rate, full = read_wav(' '.join(split[:-2]))
    return rate, full[int(begin * rate):int(end * rate)]
