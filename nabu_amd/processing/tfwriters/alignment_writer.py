"""AlignmentWriter (reference: nabu/processing/tfwriters/alignment_writer.py:8-27): feature 'data' = the raw
int32 bytes of one utterance's frame labels (Kaldi pdf ids).

The reference leaves the metadata to processors/alignment_processor.py:60-72 (max_length,
sequence_length_histogram.npy, dim = largest label + 1); this writer keeps the same three files of its directory
up to date after every utterance, so that a set it wrote can be read by AlignmentReader as it stands."""
import os

import numpy as np

from nabu_amd.processing import tfrecord
from nabu_amd.processing.tfwriters import tfwriter


class AlignmentWriter(tfwriter.TfWriter):
    '''a TfWriter to write kaldi alignments'''

    def __init__(self, datadir):
        super(AlignmentWriter, self).__init__(datadir)
        self.datadir = datadir
        self.max_length = 0
        self.sequence_length_histogram = np.zeros(0, dtype=np.int32)
        self.dim = 0

    def _get_example(self, data):
        return tfrecord.encode_example({'data': np.asarray(data).reshape([-1]).astype(np.int32).tobytes()})

    def write(self, data, name):
        super(AlignmentWriter, self).write(data, name)
        data = np.asarray(data).reshape([-1])
        n = data.size
        self.max_length = max(self.max_length, n)
        if n >= self.sequence_length_histogram.shape[0]:
            self.sequence_length_histogram = np.concatenate(
                [self.sequence_length_histogram, np.zeros(n - self.sequence_length_histogram.shape[0] + 1, np.int32)])
        self.sequence_length_histogram[n] += 1
        if n:
            self.dim = max(self.dim, int(data.max()) + 1)
        self.write_metadata()

    def write_metadata(self):
        '''the files alignment_processor.py:60-72 writes: max_length, sequence_length_histogram.npy, dim'''
        with open(os.path.join(self.datadir, 'max_length'), 'w') as fid:
            fid.write(str(self.max_length))
        np.save(os.path.join(self.datadir, 'sequence_length_histogram.npy'), self.sequence_length_histogram)
        with open(os.path.join(self.datadir, 'dim'), 'w') as fid:
            fid.write(str(self.dim))
