"""Self-attention encoder (`encoder = transformer`): the second encoder ESPnet puts behind its VGG2L front end, and the
first one of this project without a sequential dimension (Vaswani et al. 2017; pre-norm blocks as in ESPnet and Lingvo).

Per input: augment() (input_noise, SpecAugment), frontend() when `conv_channels` is set (the returned lengths are then
the pooled ones, as for dblstm), a linear layer to D = num_units (embed/{weights,biases}), sinusoidal positions (the
table is computed once on the host in float64, kept on the device, added by nabu_add_positions_f32), `num_layers`
layer.self_attention_block's (block<i>/...), a final layer norm (final_ln/{gamma,beta}) and mask_time_: frames past a
length are zero in the result and take no gradient.

cfg keys: num_layers, num_units (D), num_heads, ff_units, dropout (keep probability, on the two sublayer outputs of a
block), attention_dropout (KEEP probability of the dropout on the attention probabilities, like `dropout`: ESPnet's
1 - attention_dropout_rate, Lingvo's 1 - atten_dropout_prob; 1.0 when the key is absent; applied in training only, inside
the attention kernels, one more draw per block), input_noise, gemm_precision (the dense products), attention_precision (`f32`,
the default when the key is absent: the attention is exact fp32, self_attn.hip | `bf16`: its four products run on the
bf16 matrix pipe, self_attn_bf16.hip), attention_chunk and attention_left_chunks (a frame attends to its own chunk of
attention_chunk frames and attention_left_chunks chunks to its left, inside the attention kernels, in training and in
evaluation alike: they describe the model; absent: the whole utterance, and -1 = all chunks to the left; the frames are
those the attention sees, the pooled ones with conv_channels; attention_chunk = 1 is causal attention), the SpecAugment keys and conv_channels / feature_blocks (listener.py).  Refused at
construction: num_units not divisible by num_heads, a head width other than 32 or 64 (self_attn.hip), any other value of
attention_precision, an attention_dropout that is no finite number in (0, 1], an attention_chunk that is no integer >= 1, an
attention_left_chunks that is no integer >= -1 or comes without attention_chunk, and the keys `layer_norm` and `recurrent_precision`, which mean nothing here."""
import numpy as np
import torch

from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, requires_grad, SeqLen
from nabu_amd.neuralnetworks.components import layer
from nabu_amd.neuralnetworks.models.ed_encoders import ed_encoder
from nabu_amd.neuralnetworks.models.ed_encoders.listener import augment, conv_channels_key, frontend, spec_augment_keys

_TABLES = {}


def position_table(T, D, device):
    """pe [>= T, D] on the device: pe[t, 2i] = sin(t / 10000^(2i/D)), pe[t, 2i+1] = cos(same), from float64"""
    key = (str(device), D)
    if key not in _TABLES or _TABLES[key].shape[0] < T:
        rows = max(T, 256)
        angle = np.arange(rows, dtype=np.float64)[:, None] / 10000.0 ** (2 * (np.arange(D) // 2) / float(D))
        pe = np.where(np.arange(D) % 2 == 0, np.sin(angle), np.cos(angle))
        _TABLES[key] = torch.from_numpy(pe.astype(np.float32)).to(device)
    return _TABLES[key]


def embed(x, lens, D, precision):
    """x [B,T,F] -> x W + b + positions, [B,T,D]; variables embed/{weights,biases}"""
    B, T, F = x.shape
    with vs.variable_scope('embed'):
        W = vs.get_variable('weights', [F, D])
        b = vs.get_variable('biases', [D], initializer=vs.zeros)
    x2 = (x if x.is_contiguous() else x.contiguous()).view(B * T, F)
    y = hip.gemm(x2, W.data, torch.empty((B * T, D), dtype=torch.float32, device=x.device), bias=b.data,
                 precision=precision).view(B, T, D)
    hip.add_positions_(y, position_table(T, D, x.device), lens.dev)
    need_dx = requires_grad(x)

    def backward(dy):
        dy = dy.reshape(B * T, D).contiguous()                    # (the positions' gradient is the identity)
        for v in (W, b):
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)
        hip.gemm(x2, dy, W.grad, trans_a=True, precision=precision)
        hip.colsum(dy, b.grad)
        if not need_dx:
            return [None]
        return [hip.gemm(dy, W.data, torch.empty_like(x2), trans_b=True, precision=precision).view(B, T, F)]
    record([x], [y], backward, params=(W, b))
    return y


def final_norm(x, lens):
    """layer norm per frame (final_ln/{gamma,beta}), then frames past a length zeroed, forward and backward"""
    B, T, D = x.shape
    with vs.variable_scope('final_ln'):
        gamma = vs.get_variable('gamma', [D], initializer=vs.ones)
        beta = vs.get_variable('beta', [D], initializer=vs.zeros)
    x2 = x.view(B * T, D)
    y, mean, rstd = hip.layer_norm_fwd(x2, gamma.data, beta.data, layer.LN_EPS)
    y = hip.mask_time_(y.view(B, T, D), lens.dev)

    def backward(dy):
        dy = hip.mask_time_(dy.reshape(B, T, D).clone(), lens.dev).view(B * T, D)
        for v in (gamma, beta):
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)
        dx, dgp, dbp = hip.layer_norm_bwd(x2, gamma.data, dy, mean, rstd)
        hip.colsum(dgp, gamma.grad)
        hip.colsum(dbp, beta.grad)
        return [dx.view(B, T, D)]
    record([x], [y], backward, params=(gamma, beta))
    return y


def attention_precision_key(conf):
    """the `attention_precision` cfg key (a build addition like layer_norm: absent from the defaults files, f32 when absent)"""
    value = str(conf.get('attention_precision', 'f32')).strip()
    if value not in ('f32', 'bf16'):
        raise ValueError("transformer encoder: attention_precision must be 'f32' or 'bf16', got %r" % value)
    return value


def attention_dropout_key(conf):
    """the `attention_dropout` cfg key: the KEEP probability of the dropout on the attention probabilities, like `dropout`
    (a build addition like attention_precision: absent from the defaults files, 1.0 when absent)"""
    text = str(conf.get('attention_dropout', '1.0')).strip()
    try:
        value = float(text)
    except ValueError:
        value = float('nan')
    if not (np.isfinite(value) and 0 < value <= 1):
        raise ValueError('transformer encoder: attention_dropout is a keep probability, a number in (0, 1]; got %r' % text)
    return value


def attention_window_key(conf):
    """the `attention_chunk` and `attention_left_chunks` cfg keys (build additions, absent from the defaults files): None
    without attention_chunk, else (chunk, left_chunks) with left_chunks = -1 (all chunks to the left) when absent"""
    def integer(key, least):
        text = str(conf[key]).strip()
        try:
            value = int(text)
        except ValueError:
            value = least - 1
        if value < least:
            raise ValueError('transformer encoder: %s must be an integer >= %d, got %r' % (key, least, text))
        return value
    if 'attention_chunk' not in conf:
        if 'attention_left_chunks' in conf:
            raise ValueError('transformer encoder: attention_left_chunks counts chunks of attention_chunk frames, which is not set')
        return None
    return integer('attention_chunk', 1), integer('attention_left_chunks', -1) if 'attention_left_chunks' in conf else -1


class Transformer(ed_encoder.EDEncoder):
    """cfg keys: see the module's docstring"""

    def __init__(self, conf, constraint, name=None):
        super(Transformer, self).__init__(conf, constraint, name)
        for key in ('layer_norm', 'recurrent_precision'):
            if key in self.conf:
                raise ValueError('transformer encoder: the key %s belongs to the recurrent encoders and means nothing here' % key)
        conv_channels_key(self.conf)
        spec_augment_keys(self.conf)
        units, heads = int(self.conf['num_units']), int(self.conf['num_heads'])
        if heads < 1 or units % heads:
            raise ValueError('transformer encoder: num_units = %d is not divisible by num_heads = %d' % (units, heads))
        if units // heads not in (32, 64) or units > 1024:
            raise ValueError('transformer encoder: num_units / num_heads = %d: the attention kernels take a head width of '
                             '32 or 64 and at most 1024 units' % (units // heads))
        attention_precision_key(self.conf)
        attention_dropout_key(self.conf)
        self.attention_window = attention_window_key(self.conf)

    def encode(self, inputs, input_seq_length, is_training):
        layer.GEMM_PRECISION[0] = precision = self.conf.get('gemm_precision', 'default')
        layer.ATTENTION_PRECISION[0] = attention_precision_key(self.conf)
        units, heads, ff = (int(self.conf[k]) for k in ('num_units', 'num_heads', 'ff_units'))
        keep = float(self.conf['dropout'])
        self.attention_keep = attention_dropout_key(self.conf) if is_training else 1.0
        encoded, encoded_seq_length = {}, dict(input_seq_length)
        for name, x in inputs.items():
            with vs.variable_scope(name):
                x, lengths = augment(self.conf, x, input_seq_length[name], is_training)
                if conv_channels_key(self.conf):
                    x, lengths = frontend(self.conf, x, lengths)
                    encoded_seq_length[name] = lengths
                lens = SeqLen.wrap(lengths, x.device)
                x = embed(x, lens, units, precision)
                for index in range(int(self.conf['num_layers'])):
                    x = self.block(x, lens, heads, ff, keep if is_training else 1.0, 'block%d' % index)
                encoded[name] = final_norm(x, lens)
        return encoded, encoded_seq_length

    def block(self, x, lens, heads, ff, keep, scope):
        """one block of the stack (conformer.py puts its own here)"""
        return layer.self_attention_block(x, lens, heads, ff, keep, scope=scope, attention_keep=self.attention_keep,
                                          attention_window=self.attention_window)
