"""Listener: a stack of pyramidal BLSTM layers topped by one plain BLSTM layer (the role of
nabu/neuralnetworks/models/ed_encoders/listener.py:14-74).  Each layer is ONE call into the C ABI
(layer.blstm -> nabu_blstm_fwd); the pyramid stacking between layers is a view of the batch-major
output buffer."""
from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.components import layer, ops
from nabu_amd.neuralnetworks.models.ed_encoders import ed_encoder


def layer_norm_key(conf):
    """the `layer_norm` cfg key (a build addition like gemm_precision: absent from the defaults file, False when absent)"""
    value = str(conf.get('layer_norm', 'False')).strip()
    if value not in ('True', 'False'):
        raise ValueError("layer_norm must be 'True' or 'False', got %r" % value)
    return value == 'True'


SPEC_AUGMENT_KEYS = ('time_warp', 'time_masks', 'time_mask_width', 'time_mask_ratio', 'freq_masks', 'freq_mask_width',
                     'feature_blocks')


def spec_augment_keys(conf):
    """the SpecAugment cfg keys of the [encoder] section (build additions like layer_norm: absent from the defaults
    files, everything off when absent) as a hip.SpecAugmentPolicy:
      time_warp W (0: off), time_masks (0: off) of 0..time_mask_width frames, no wider than time_mask_ratio (default
      1.0) of the utterance, freq_masks (0: off) of 0..freq_mask_width columns, feature_blocks (default 1) equal
      column blocks that a frequency mask repeats in (3 for ddelta features).
    That feature_blocks divides the feature dimension is checked where the features are seen (ops.spec_augment)."""
    def integer(key, default, low=0, high=None):
        text = str(conf.get(key, default)).strip()
        try:
            value = int(text)
        except ValueError:
            raise ValueError('%s must be an integer, got %r' % (key, text))
        if value < low or (high is not None and value > high):
            raise ValueError('%s must be %s, got %d' % (key, '>= %d' % low if high is None else 'in %d..%d' % (low, high),
                                                        value))
        return value
    text = str(conf.get('time_mask_ratio', '1.0')).strip()
    try:
        ratio = float(text)
    except ValueError:
        raise ValueError('time_mask_ratio must be a number, got %r' % text)
    if not 0.0 < ratio <= 1.0:
        raise ValueError('time_mask_ratio must be in (0, 1], got %r' % text)
    return hip.SpecAugmentPolicy(
        time_warp=integer('time_warp', 0, high=(1 << 24) - 1),
        time_masks=integer('time_masks', 0, high=hip.SPECAUG_MAX_MASKS),
        time_mask_width=integer('time_mask_width', 0), time_mask_ratio=ratio,
        freq_masks=integer('freq_masks', 0, high=hip.SPECAUG_MAX_MASKS),
        freq_mask_width=integer('freq_mask_width', 0), feature_blocks=integer('feature_blocks', 1, low=1))


def augment(conf, x, lengths, is_training):
    """the encoders' input regularisation: input_noise, then SpecAugment (its own RngState.next(), after the noise's, so
    that a configuration without the new keys keeps its offsets); the lengths come back as the SeqLen the kernel read"""
    noise = float(conf['input_noise'])
    policy = spec_augment_keys(conf)
    if is_training and noise > 0:                                       # listener.py:40-45, dblstm.py:37-42
        x = ops.input_noise(x, noise, ops.global_rng())
    if is_training and policy.on:
        lengths = SeqLen.wrap(lengths, x.device)
        x = ops.spec_augment(x, lengths, policy, ops.global_rng())
    return x, lengths


class Listener(ed_encoder.EDEncoder):
    """cfg keys: num_layers (pyramidal layers), num_units, pyramid_steps, input_noise, dropout (keep
    probability), gemm_precision (build addition), layer_norm (build addition, default False: every layer's cells
    normalise their gates and state — layer.blstm(layer_norm=True)), the SpecAugment keys (build additions, default
    off: spec_augment_keys)"""

    def _regularise(self, x, is_training):
        keep = float(self.conf['dropout'])
        return ops.seq_dropout(x, keep, ops.global_rng()) if (is_training and keep < 1) else x

    def _encode_one(self, x, lengths, is_training):
        x, lengths = augment(self.conf, x, lengths, is_training)
        units, depth = int(self.conf['num_units']), int(self.conf['num_layers'])
        layer_norm = layer_norm_key(self.conf)
        for index in range(depth):                                      # listener.py:49-59
            x, lengths = layer.pblstm(inputs=x, sequence_length=lengths, num_units=units,
                                      num_steps=int(self.conf['pyramid_steps']), layer_norm=layer_norm,
                                      scope='layer%d' % index)
            x = self._regularise(x, is_training)
        x = layer.blstm(inputs=x, sequence_length=lengths, num_units=units, layer_norm=layer_norm,
                        scope='layer%d' % depth)                                       # :61-65
        return self._regularise(x, is_training), lengths

    def encode(self, inputs, input_seq_length, is_training):
        # arithmetic of the input-to-hidden GEMMs of the layers built below (BASELINE.json configs[4]
        # asks for bf16 MFMA there); 'default' = the process default = exact fp32
        layer.GEMM_PRECISION[0] = self.conf.get('gemm_precision', 'default')
        layer.RECURRENT_PRECISION[0] = self.conf.get('recurrent_precision', 'default')
        encoded, encoded_seq_length = {}, {}
        for name, x in inputs.items():
            with vs.variable_scope(name):
                encoded[name], encoded_seq_length[name] = self._encode_one(x, input_seq_length[name], is_training)
        return encoded, encoded_seq_length
