"""TextProcessor (reference: nabu/processing/processors/text_processor.py:9-92): normalises a transcription
and keeps the metadata string readers need.  Host string work only."""
import os

import numpy as np

from nabu_amd.processing.processors import processor
from nabu_amd.processing.target_normalizers import normalizer_factory


class TextProcessor(processor.Processor):
    '''a processor for text data, does normalization'''

    def __init__(self, conf):
        self.normalizer = normalizer_factory.factory(conf.get('processor', 'normalizer'))
        alphabet = conf.get('processor', 'alphabet').strip().split(' ')
        self.alphabet = [c if c != '\\;' else ';' for c in alphabet]     # ';' starts a comment in a cfg
        self.max_length = 0
        self.sequence_length_histogram = np.zeros(0, dtype=np.int32)
        super(TextProcessor, self).__init__(conf)
        self.nonesymbol = '' if self.conf['nonesymbol'] == 'None' else self.conf['nonesymbol']

    def __call__(self, dataline):
        '''the normalized transcription as a space separated string, or None when it is longer than max_length'''
        normalized = self.normalizer(dataline, self.alphabet + [self.nonesymbol])
        seq_length = len(normalized.split(' '))
        max_length = self._max_length()
        if max_length is not None and seq_length > max_length:
            return None
        self._count(seq_length)
        return normalized

    def write_metadata(self, datadir):
        with open(os.path.join(datadir, 'max_length'), 'w') as fid:
            fid.write(str(self.max_length))
        with open(os.path.join(datadir, 'sequence_length_histogram.npy'), 'wb') as fid:
            np.save(fid, self.sequence_length_histogram)
        with open(os.path.join(datadir, 'alphabet'), 'w') as fid:
            fid.write(' '.join(self.alphabet))
        with open(os.path.join(datadir, 'dim'), 'w') as fid:
            fid.write(str(len(self.alphabet)))
        with open(os.path.join(datadir, 'nonesymbol'), 'w') as fid:
            fid.write(self.nonesymbol)
