"""AlignmentReader (reference: nabu/processing/tfreaders/alignment_reader.py:9-72): 'data' = the raw int32 bytes
of the frame labels; the sequence length is their count.  Metadata: max_length and sequence_length_histogram.npy."""
import numpy as np

from nabu_amd.processing.tfreaders import tfreader


class AlignmentReader(tfreader.TfReader):
    '''reader for kaldi alignments'''

    def _read_metadata(self, datadirs):
        metadata = dict()
        self._lengths(datadirs, metadata)
        return metadata

    def sequence_length(self, filename):
        '''frames = bytes of the 'data' feature / 4, read from the record's length prefixes'''
        from nabu_amd.processing import tfrecord
        n = tfrecord.peek_single_bytes_feature(filename, 'data')
        if n is None or n % 4:
            return super(AlignmentReader, self).sequence_length(filename)
        return n // 4

    def _process_features(self, features):
        data = np.frombuffer(features['data'][0], np.int32).copy()
        return data, data.shape[0]
