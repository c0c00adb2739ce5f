"""Target normalizers by name (the role of nabu/processing/target_normalizers/normalizer_factory.py);
the result is a function (transcription, alphabet) -> string."""
from nabu_amd.tools.registry import Registry

factory = Registry('normalizer', {
    'phones': 'nabu_amd.processing.target_normalizers.phones:normalize',
}, outside=('aurora4', 'character', 'gp'), undefined='Undefined %s: %s')
