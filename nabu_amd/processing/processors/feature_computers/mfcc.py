"""Mel frequency cepstral coefficients (reference: .../feature_computers/mfcc.py:9-55)."""
from nabu_amd.processing.processors.feature_computers import feature_computer


class Mfcc(feature_computer.FeatureComputer):
    '''the feature computer class to compute MFCC features'''
    kind = 'mfcc'

    def _num_static(self):
        return int(self.conf['numcep'])
