"""Feature computers by name (the role of .../feature_computers/feature_computer_factory.py)."""
from nabu_amd.tools.registry import Registry

_PKG = 'nabu_amd.processing.processors.feature_computers.'
factory = Registry('feature', {
    'fbank': _PKG + 'fbank:Fbank',
    'mfcc': _PKG + 'mfcc:Mfcc',
}, outside=('ssc', 'raw'), undefined='Undefined %s type: %s')
