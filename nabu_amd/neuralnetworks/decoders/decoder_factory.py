"""Decoder classes by recipe name (the role of nabu/neuralnetworks/decoders/decoder_factory.py:4-37)."""
from nabu_amd.tools.registry import Registry

factory = Registry('decoder', {
    'ctc_decoder': 'nabu_amd.neuralnetworks.decoders.ctc_decoder:CTCDecoder',
    'beam_search_decoder': 'nabu_amd.neuralnetworks.decoders.beam_search_decoder:BeamSearchDecoder',
    'alignment_decoder': 'nabu_amd.neuralnetworks.decoders.alignment_decoder:AlignmentDecoder',
    'random_decoder': 'nabu_amd.neuralnetworks.decoders.random_decoder:RandomDecoder',
    'ctc_alignment_decoder': 'nabu_amd.neuralnetworks.decoders.ctc_alignment_decoder:CTCAlignmentDecoder',
    'transducer_decoder': 'nabu_amd.neuralnetworks.decoders.transducer_decoder:TransducerDecoder',
    'transducer_alignment_decoder':
        'nabu_amd.neuralnetworks.decoders.transducer_alignment_decoder:TransducerAlignmentDecoder',
}, outside=('max_decoder', 'threshold_decoder', 'feature_decoder'),
    undefined='Undefined %s type: %s')
