"""Conformer encoder (`encoder = conformer`; Gulati et al. 2020): the self-attention encoder of transformer.py with
layer.conformer_block in place of layer.self_attention_block — macaron half-step feed-forward layers with Swish around
the attention and a convolution module (conv_module.hip: GLU, depthwise convolution along time, norm, Swish between two
pointwise products).  augment(), frontend(), embed(), the position table and final_norm() are the transformer's.

The module's norm is a layer norm per frame (WeNet's `cnn_module_norm: layer_norm`, NeMo's `conv_norm_type: layer_norm`),
not the paper's batch norm: batch statistics over a ragged padded batch would make an utterance's result depend on its
neighbours, and would add running averages outside the parameter buffer.

cfg keys: the transformer's (attention_chunk / attention_left_chunks limit the attention only: the convolution module
still reads (conv_kernel - 1) / 2 frames ahead), and conv_kernel (taps of the depthwise convolution: odd, 3..31), which the [encoder] section
must set itself.  Refused at construction: everything Transformer refuses, num_units not a multiple of 64, and a missing,
even or out-of-range conv_kernel."""
from nabu_amd.neuralnetworks.components import layer
from nabu_amd.neuralnetworks.models.ed_encoders.transformer import Transformer


class Conformer(Transformer):
    """cfg keys: see the module's docstring"""

    def __init__(self, conf, constraint, name=None):
        if not conf.has_option('encoder', 'conv_kernel'):
            raise ValueError('conformer encoder: the [encoder] section sets no conv_kernel (odd, 3..31)')
        super(Conformer, self).__init__(conf, constraint, name)
        if int(self.conf['num_units']) % 64:
            raise ValueError('conformer encoder: num_units = %s is not a multiple of 64 (conv_module.hip)' % self.conf['num_units'])
        kernel = int(self.conf['conv_kernel'])
        if kernel % 2 == 0 or not 3 <= kernel <= 31:
            raise ValueError('conformer encoder: conv_kernel = %d, must be odd in 3..31' % kernel)

    def block(self, x, lens, heads, ff, keep, scope):
        return layer.conformer_block(x, lens, heads, ff, int(self.conf['conv_kernel']), keep, scope=scope,
                                     attention_keep=self.attention_keep, attention_window=self.attention_window)
