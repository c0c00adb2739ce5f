"""Log mel filterbank features (reference: .../feature_computers/fbank.py:9-55)."""
from nabu_amd.processing.processors.feature_computers import feature_computer


class Fbank(feature_computer.FeatureComputer):
    '''the feature computer class to compute fbank features'''
    kind = 'fbank'

    def _num_static(self):
        return int(self.conf['nfilt'])
