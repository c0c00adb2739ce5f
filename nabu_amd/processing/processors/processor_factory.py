"""Processors by name (the role of nabu/processing/processors/processor_factory.py)."""
from nabu_amd.tools.registry import Registry

_PKG = 'nabu_amd.processing.processors.'
factory = Registry('processor', {
    'audio_processor': _PKG + 'audio_processor:AudioProcessor',
    'text_processor': _PKG + 'text_processor:TextProcessor',
}, outside=('binary_processor', 'alignment_processor', 'textfile_processor'), undefined='unknown %s type: %s')
