"""Neural network layers (reference: nabu/neuralnetworks/components/layer.py).

Same functions, same variable names; the body of ``blstm`` is ONE call into the
C ABI (nabu_blstm_fwd) instead of two tf.while_loops of ~15 small ops per step."""
import torch

from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, requires_grad, SeqLen, Tape
from nabu_amd.neuralnetworks.components import ops

# cell scope of tf.contrib.rnn.LayerNormBasicLSTMCell under bidirectional_dynamic_rnn
_CELL = 'bidirectional_rnn/%s/layer_norm_basic_lstm_cell'
LSTM_MODE = [hip.LSTM_AUTO]      # tests flip this to compare the two recurrent paths
# arithmetic of the input-to-hidden GEMMs of the layers built next ('default' | 'f32' | 'bf16' |
# 'bf16x3' | 'bf16x6'); set by the encoders from their `gemm_precision` cfg key
GEMM_PRECISION = ['default']
# arithmetic of the attention products of the self-attention and conformer blocks built next ('f32' = self_attn.hip |
# 'bf16' = self_attn_bf16.hip, the four products on the bf16 matrix pipe); set by the transformer encoder from its
# `attention_precision` cfg key
ATTENTION_PRECISION = ['f32']
# arithmetic of the recurrent product h.W_h of the layers built next ('default' = three fp16 plane products of row-scaled
# operands, fp32-equivalent | 'f32' = the exact-fp32 kernels); set by the encoders from their `recurrent_precision` key
RECURRENT_PRECISION = ['default']
# the weight-gradient products of a layer run after the LAST recurrence of the backward pass (Tape.defer): nothing
# waits for them, and bf16 matrix bursts in front of a persistent recurrent kernel slow it down (include/nabu_hip.h,
# nabu_blstm_bwd_data).  NABU_DEFER_WGRAD=0: one fused nabu_blstm_bwd per layer as before.
import os as _os
DEFER_WEIGHT_GRADS = [_os.environ.get('NABU_DEFER_WGRAD', '1') != '0']
# tests: a list here receives, per layer and backward pass, the operands of the layer's dense products (x, out, the
# kernels and a copy of dz as the data part of the backward pass left it in the reserve) — tests/test_hip_real_operands.py
CAPTURE = [None]


# packed companions (include/nabu_hip.h, ABI version 3): the forward recurrent kernel writes the layer's output also as the
# next layer's f16x3 operands and its own h^T operand.  NABU_PACKED_COMPANIONS=0: every call packs for itself as before.
PACKED_COMPANIONS = [_os.environ.get('NABU_PACKED_COMPANIONS', '1') != '0']
# NABU_CHECK_X_BOUND=1: every layer call measures max|x| (host round trip) and raises if it exceeds the bound it was promised
CHECK_X_BOUND = [_os.environ.get('NABU_CHECK_X_BOUND', '0') == '1']


def layer_norm_variable_names(direction):
    """names of one direction's variables of a layer-normalised cell, relative to the layer's scope: kernel, then
    gamma and beta of the norm scopes in ABI order (hip.LN_SCOPES); there is no bias"""
    cell = _CELL % direction
    return [cell + '/kernel'] + ['%s/%s/%s' % (cell, s, w) for s in hip.LN_SCOPES for w in ('gamma', 'beta')]


def _plain_cell(D, H):
    """the plain cell's variables and entry points: (plan class, variables, the two kernels, fwd, bwd_data, bwd).  The three calls take
    (plan, x, lens, ...) up to the point where the cells' argument lists part: fwd(..., out, reserve),
    bwd_data(..., out, dout, reserve, dx), bwd(..., out, dout, reserve, dx) — the latter two write v.grad"""
    kf = vs.get_variable((_CELL % 'fw') + '/kernel', [D + H, 4 * H])
    bf = vs.get_variable((_CELL % 'fw') + '/bias', [4 * H])
    kb = vs.get_variable((_CELL % 'bw') + '/kernel', [D + H, 4 * H])
    bb = vs.get_variable((_CELL % 'bw') + '/bias', [4 * H])

    def fwd(plan, x, lens, out, reserve):
        hip.blstm_fwd(plan, x, lens, kf.data, bf.data, kb.data, bb.data, out, reserve)

    def bwd_data(plan, x, lens, out, dout, reserve, dx):
        hip.blstm_bwd_data(plan, x, lens, kf.data, kb.data, out, dout, reserve, dx, bf.grad, bb.grad)

    def bwd(plan, x, lens, out, dout, reserve, dx):
        hip.blstm_bwd(plan, x, lens, kf.data, kb.data, out, dout, reserve, dx, kf.grad, bf.grad, kb.grad, bb.grad)
    return hip.BlstmPlan, (kf, bf, kb, bb), (kf, kb), fwd, bwd_data, bwd


def _layer_norm_cell(D, H):
    """... of LayerNormBasicLSTMCell(layer_norm=True) (include/nabu_hip.h, nabu_blstm_ln_fwd).  Variables per direction
    under the same cell scope: kernel [(D+H),4H] (scope-default initialiser) and
    {input,transform,forget,output,state}/{gamma,beta} [H] (1 / 0); NO bias.  The exact-fp32 stepwise kernels:
    LSTM_MODE = PERSISTENT is refused, recurrent_precision has nothing to select, no packed companions are attached (the
    consumer packs for itself)."""
    if LSTM_MODE[0] == hip.LSTM_PERSISTENT:
        raise hip._hip.NabuHipError('blstm(layer_norm=True) with LSTM_MODE = PERSISTENT: the persistent recurrent kernels '
                                    'split the units of a row over workgroups and have no per-step reduction across them; '
                                    'layer norm runs in the stepwise family (LSTM_AUTO or LSTM_STEPWISE)')
    kernels, gammas, betas = [], [], []
    for direction in ('fw', 'bw'):
        names = layer_norm_variable_names(direction)
        kernels.append(vs.get_variable(names[0], [D + H, 4 * H]))
        # (created in the cell's order: per norm scope gamma, then beta)
        norms = [vs.get_variable(n, [H], initializer=vs.ones if n.endswith('gamma') else vs.zeros) for n in names[1:]]
        gammas.append(norms[0::2])
        betas.append(norms[1::2])
    kf, kb = kernels

    def data(group):
        return [[v.data for v in vars_] for vars_ in group]

    def grads(group):
        return [[v.grad for v in vars_] for vars_ in group]

    def fwd(plan, x, lens, out, reserve):
        hip.blstm_ln_fwd(plan, x, lens, kf.data, kb.data, data(gammas), data(betas), out, reserve)

    def bwd_data(plan, x, lens, out, dout, reserve, dx):
        hip.blstm_ln_bwd_data(plan, x, lens, kf.data, kb.data, data(gammas), data(betas), out, dout, reserve, dx,
                              grads(gammas), grads(betas))

    def bwd(plan, x, lens, out, dout, reserve, dx):
        hip.blstm_ln_bwd(plan, x, lens, kf.data, kb.data, data(gammas), data(betas), out, dout, reserve, dx, kf.grad, kb.grad,
                         grads(gammas), grads(betas))
    return hip.BlstmLnPlan, tuple([kf, kb] + gammas[0] + gammas[1] + betas[0] + betas[1]), (kf, kb), fwd, bwd_data, bwd


def _attach_companions(plan, inputs, x, training, scope, out_stack):
    """packed companions of a plain layer (PACKED_COMPANIONS): attaches what the producer wrote of the input and what
    this layer's recurrent kernel writes itself; returns the output's pair for the consumer, or None"""
    B, T, D, H = plan.desc.B, plan.desc.T, plan.desc.D, plan.desc.H
    # input: the producer layer's kernel wrote it (ops.packed), if this layer's products read packed operands at all
    x_pk = ops.packed(inputs, 1) if x is inputs else None
    if x_pk is not None and plan.pk_bytes[0] and (x_pk[0].numel(), x_pk[1].numel()) == tuple(plan.pk_bytes[:2]):
        hip.blstm_set_companions(plan, x_pk=x_pk)
    # output, for the consumer behind `out_stack` stacked frames: only if that layer (same units, same arithmetic)
    # would read them
    want_out = False
    if out_stack in (1, 2) and T % out_stack == 0 and plan.pk_bytes[3]:
        nxt = hip.BlstmPlan(B, T // out_stack, 2 * H * out_stack, H, T // out_stack, LSTM_MODE[0], GEMM_PRECISION[0], x_bound=1.0,
                            fwd_only=not training, recurrent_precision=RECURRENT_PRECISION[0])
        want_out = nxt.pk_bytes[0] == plan.pk_bytes[3] and nxt.pk_bytes[1] == plan.pk_bytes[4]
    # only what the recurrent kernel writes itself is attached; the rest is packed where it is needed, as before.  A
    # buffer stays busy while its holders (this plan, `out`, the consumer's plan) are alive (ops.BufferPool)
    mask = hip.blstm_emits_packed(plan, out_pk=want_out, hT_pk=training and plan.pk_bytes[2] > 0)

    def acquire(role, i):
        return ops.companions.acquire((vs.current_scope(), scope or 'BLSTM', role), plan.pk_bytes[i], x.device, (B, T, D, H))
    out_pk = (acquire('rows', 3), acquire('cols', 4)) if mask & 3 == 3 else None
    hip.blstm_set_companions(plan, out_pk=out_pk, hT_pk=acquire('hT', 2) if mask & 4 else None)
    return out_pk


def blstm(inputs, sequence_length, num_units, layer_norm=False, scope=None, out_stack=0):
    """A BLSTM layer (reference layer.py:8-51).

    inputs [B,T,D] fp32 contiguous on the GPU; sequence_length [B];
    returns [B,T,2*num_units] = concat(fw, bw).  Variables (TF layout):
    <scope>/bidirectional_rnn/{fw,bw}/layer_norm_basic_lstm_cell/{kernel [(D+H),4H], bias [4H]},
    gate order i,j,f,o; both use the scope-default glorot-uniform initialiser.  layer_norm: _layer_norm_cell."""
    lens = SeqLen.wrap(sequence_length, inputs.device)
    B, T, D = inputs.shape
    H = int(num_units)
    with vs.variable_scope(scope or 'BLSTM'):
        Plan, variables, kernels, fwd, bwd_data, bwd = (_layer_norm_cell if layer_norm else _plain_cell)(D, H)
    # what is known about the input's magnitude (ops.value_bound: the previous layer's outputs, |o tanh c| <= 1, through
    # pyramid stacking and dropout) spares the f16x3 packs of x their measuring pass; no tape = no backward pass: the
    # reserve then holds the activations only
    training = Tape.current is not None
    plan = Plan(B, T, D, H, min(lens.max(), T), LSTM_MODE[0], GEMM_PRECISION[0], x_bound=ops.value_bound(inputs),
                fwd_only=not training, recurrent_precision=RECURRENT_PRECISION[0], out_stack=out_stack)
    x = inputs if inputs.is_contiguous() else inputs.contiguous()
    if not layer_norm and CHECK_X_BOUND[0] and ops.value_bound(inputs) > 0:
        # debug mode (NABU_CHECK_X_BOUND=1): the recorded bound is a PROMISE (ops.set_value_bound) — an in-place change
        # of a bounded tensor would leave it stale and the f16x3 packs would overflow to Inf without a diagnostic
        worst = float(x.detach().cpu().numpy().__abs__().max())
        if not worst <= ops.value_bound(inputs) * (1 + 1e-6):
            raise RuntimeError('blstm input exceeds its recorded bound: max|x| = %g > %g (a tensor carrying a value bound '
                               'was modified in place?)' % (worst, ops.value_bound(inputs)))
    out_pk = _attach_companions(plan, inputs, x, training, scope, out_stack) if PACKED_COMPANIONS[0] and not layer_norm else None
    out = torch.empty((B, T, 2 * H), dtype=torch.float32, device=x.device)
    reserve = torch.empty(plan.reserve_bytes, dtype=torch.uint8, device=x.device)
    fwd(plan, x, lens.dev, out, reserve)
    ops.set_value_bound(out, 1.0)           # |tanh(c) sigmoid(o)| <= 1, with layer norm as well
    if out_pk is not None:
        ops.set_packed(out, out_stack, out_pk)
    need_dx = requires_grad(inputs)

    def backward(dout):
        for v in variables:
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)
        dx = torch.empty_like(x) if need_dx else None
        tape = Tape.current_backward
        if DEFER_WEIGHT_GRADS[0] and tape is not None:
            bwd_data(plan, x, lens.dev, out, dout.contiguous(), reserve, dx)
            if CAPTURE[0] is not None and not layer_norm:
                kf, bf, kb, bb = variables
                n = B * T * 4 * H
                dz = reserve[:2 * n * 4].view(torch.float32).view(2, B * T, 4 * H).clone()
                CAPTURE[0].append({'x': x, 'out': out, 'kf': kf.data, 'kb': kb.data, 'dz': dz, 'B': B, 'T': T, 'D': D, 'H': H,
                                   'bf': bf.data, 'bb': bb.data, 'lens': lens.dev.cpu().numpy(), 'dout': dout.contiguous().clone()})
            tape.defer(lambda: hip.blstm_bwd_weights(plan, x, lens.dev, out, reserve, kernels[0].grad, kernels[1].grad),
                       params=kernels)
        else:
            bwd(plan, x, lens.dev, out, dout.contiguous(), reserve, dx)
        return [dx]
    record([inputs], [out], backward, params=variables)
    return out


def conv_block(inputs, sequence_length, channels, in_channels, scope=None):
    """One block of the convolutional front end (Zhang, Chan and Jaitly 2017; ESPnet's VGG2L): two 3x3 convolutions
    with ReLU, then a 2x2 max-pool in ceil mode, as ONE tape node (conv2d.hip).

    inputs [B,T,F,in_channels] channels-last fp32; returns ([B,ceil(T/2),ceil(F/2),channels], SeqLen of ceil(len/2)).
    Variables: <scope>/conv{0,1}/kernel [3,3,Cin,channels] (scope-default initialiser), conv{0,1}/bias (zeros).
    Frames past an utterance's length are zero in every tensor of the block (include/nabu_hip.h: the length rule)."""
    lens = SeqLen.wrap(sequence_length, inputs.device)
    C = int(channels)
    if inputs.shape[3] != in_channels:
        raise ValueError('conv_block: inputs have %d channels, in_channels = %d' % (inputs.shape[3], in_channels))
    with vs.variable_scope(scope or 'conv_block'):
        w0 = vs.get_variable('conv0/kernel', [3, 3, int(in_channels), C])
        b0 = vs.get_variable('conv0/bias', [C], initializer=vs.zeros)
        w1 = vs.get_variable('conv1/kernel', [3, 3, C, C])
        b1 = vs.get_variable('conv1/bias', [C], initializer=vs.zeros)
    variables = (w0, b0, w1, b1)
    x = inputs if inputs.is_contiguous() else inputs.contiguous()
    y0 = hip.conv3x3_relu(x, lens.dev, w0.data, b0.data)
    y1 = hip.conv3x3_relu(y0, lens.dev, w1.data, b1.data)
    out = hip.maxpool2x2(y1, lens.dev)
    need_dx = requires_grad(inputs)

    def backward(dout):
        for v in variables:
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)
        dy1 = hip.maxpool2x2_bwd(y1, lens.dev, dout.reshape(out.shape).contiguous())
        hip.conv3x3_bwd_weights(y0, dy1, y1, lens.dev, w1.grad, b1.grad)
        dy0 = hip.conv3x3_bwd_data(dy1, y1, lens.dev, w1.data)
        hip.conv3x3_bwd_weights(x, dy0, y0, lens.dev, w0.grad, b0.grad)
        # (features are leaves: the first block computes no data gradient)
        return [hip.conv3x3_bwd_data(dy0, y0, lens.dev, w0.data) if need_dx else None]
    record([inputs], [out], backward, params=variables)
    return out, ops.stacked_lengths(lens, 2)


def conv_frontend(inputs, sequence_length, channels, feature_blocks=1):
    """The VGG-style front end under the BLSTM layers: inputs [B,T,D], whose `feature_blocks` equal column blocks are
    the input channels, through one conv_block per entry of `channels` (variables frontend/block{i}/...).  Returns
    ([B,T'',F''*C], lengths) with T'' and the lengths halved (ceil) once per block, column f*C + c — the view of what
    the last pool wrote.  No value bound is attached: the consumer's packed products take their own maxima."""
    if inputs.shape[2] % feature_blocks:
        raise ValueError('feature_blocks = %d does not divide the feature dimension %d' % (feature_blocks, inputs.shape[2]))
    x = hip.blocks_to_channels(inputs if inputs.is_contiguous() else inputs.contiguous(), feature_blocks)
    if requires_grad(inputs):
        raise Exception('conv_frontend: the features depend on a parameter; the channel split computes no input gradient')
    lengths, cin = sequence_length, feature_blocks
    with vs.variable_scope('frontend'):
        for i, c in enumerate(channels):
            x, lengths = conv_block(x, lengths, c, cin, scope='block%d' % i)
            cin = c
    B, T2, F2, C = x.shape
    out = x.view(B, T2, F2 * C)
    record([x], [out], lambda dout: [dout.reshape(B, T2, F2, C)])
    return out, lengths


LN_EPS = 1e-5       # variance epsilon of the self-attention block's layer norms (moments per frame over D)


def self_attention_block(inputs, sequence_length, num_heads, ff_units, keep=1.0, scope=None, attention_keep=1.0,
                         attention_window=None):
    """One pre-norm self-attention block (Vaswani et al. 2017 with the norm in front, as ESPnet's and Lingvo's encoders
    run it) as ONE tape node:
        a = LN(h); qkv = a Wqkv + b (one product to 3D columns); c = self_attn(qkv); h = h + drop(c Wo + bo)
        f = LN(h); h = h + drop(relu(f W1 + b1) W2 + b2)
    inputs [B,T,D] fp32; the attention (self_attn.hip) sees the frames < sequence_length of each row only.  The products
    run at GEMM_PRECISION (nabu_gemm_ex falls back to exact fp32 where the 16-bit kernels do not take a shape), the
    attention itself at ATTENTION_PRECISION (exact fp32 unless set to 'bf16'; read once, for forward and backward call).  keep: dropout keep probability, applied under a tape only.
    attention_keep: keep probability of the dropout on the attention probabilities (ESPnet's attention_dropout_rate, Lingvo's
    atten_dropout_prob, as keep probabilities), made inside the attention kernels; under a tape and below 1 it takes ONE
    more draw from the global stream, after the block's other draws, and hands the same (seed, offset) to the forward and
    the backward call.  Without a tape no draw is taken and the plain kernels run.  Frames past a length carry finite values that no valid frame reads; the encoder masks them.
    attention_window: None (every pair of frames), or (chunk, left_chunks): a frame attends to its own chunk of `chunk` frames
    and `left_chunks` chunks to its left (-1: all), inside the kernels, with or without a tape; handed to the forward and
    the backward call.
    Variables: <scope>/{ln1,ln2}/{gamma,beta} [D], attention/{qkv,out}/{weights,biases}, ffn/{fc1,fc2}/{weights,biases}."""
    lens = SeqLen.wrap(sequence_length, inputs.device)
    B, T, D = inputs.shape
    H, FF, N = int(num_heads), int(ff_units), B * T
    if D % H or D // H not in (32, 64):
        raise ValueError('self_attention_block: %d units in %d heads; the head width must be 32 or 64' % (D, H))
    with vs.variable_scope(scope or 'self_attention_block'):
        norms = [(vs.get_variable('%s/gamma' % n, [D], initializer=vs.ones), vs.get_variable('%s/beta' % n, [D], initializer=vs.zeros))
                 for n in ('ln1', 'ln2')]
        dense = [(vs.get_variable('%s/weights' % n, [i, o]), vs.get_variable('%s/biases' % n, [o], initializer=vs.zeros))
                 for n, i, o in (('attention/qkv', D, 3 * D), ('attention/out', D, D), ('ffn/fc1', D, FF), ('ffn/fc2', FF, D))]
    variables = tuple(v for pair in norms + dense for v in pair)
    precision, attn_precision = GEMM_PRECISION[0], ATTENTION_PRECISION[0]
    training = Tape.current is not None
    rng = [ops.global_rng().next() for _ in range(2)] if training and keep < 1 else None
    attn_rng = ops.global_rng().next() if training and attention_keep < 1 else None

    def linear(x, i, width):
        W, b = dense[i]
        return hip.gemm(x, W.data, torch.empty((N, width), dtype=torch.float32, device=x.device), bias=b.data, precision=precision)

    def drop(x, i):
        return hip.dropout(x, keep, *rng[i]) if rng else x

    x = (inputs if inputs.is_contiguous() else inputs.contiguous()).view(N, D)
    a, mean1, rstd1 = hip.layer_norm_fwd(x, norms[0][0].data, norms[0][1].data, LN_EPS)
    qkv = linear(a, 0, 3 * D).view(B, T, 3 * D)
    c, lse = hip.self_attn_fwd(qkv, lens.dev, H, attn_precision, attention_keep, attn_rng, attention_window)
    h1 = hip.axpy_(drop(linear(c.view(N, D), 1, D), 0), x)
    f, mean2, rstd2 = hip.layer_norm_fwd(h1, norms[1][0].data, norms[1][1].data, LN_EPS)
    r = hip.relu(linear(f, 2, FF))
    out = hip.axpy_(drop(linear(r, 3, D), 1), h1).view(B, T, D)
    need_dx = requires_grad(inputs)

    def backward(dout):
        for v in variables:
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)

        def linear_bwd(x, dy, i):
            """gradients of dense[i] (overwritten) at input x; returns dx"""
            W, b = dense[i]
            hip.gemm(x, dy, W.grad, trans_a=True, precision=precision)
            hip.colsum(dy, b.grad)
            return hip.gemm(dy, W.data, torch.empty_like(x), trans_b=True, precision=precision)

        def norm_bwd(x, dy, i, mean, rstd):
            dx, dgp, dbp = hip.layer_norm_bwd(x, norms[i][0].data, dy, mean, rstd)
            hip.colsum(dgp, norms[i][0].grad)
            hip.colsum(dbp, norms[i][1].grad)
            return dx
        dout = dout.reshape(N, D).contiguous()
        du = hip.relu_bwd(r, linear_bwd(r, drop(dout, 1), 3))
        dh1 = hip.axpy_(norm_bwd(h1, linear_bwd(f, du, 2), 1, mean2, rstd2), dout)
        dc = linear_bwd(c.view(N, D), drop(dh1, 0), 1)
        dqkv = hip.self_attn_bwd(qkv, c, lse, dc.view(B, T, D), lens.dev, H, attn_precision, attention_keep, attn_rng,
                                 attention_window)
        da = linear_bwd(a, dqkv.reshape(N, 3 * D), 0)
        if not need_dx:                                  # (the norm's own gradients are still due)
            norm_bwd(x, da, 0, mean1, rstd1)
            return [None]
        return [hip.axpy_(norm_bwd(x, da, 0, mean1, rstd1), dh1).view(B, T, D)]
    record([inputs], [out], backward, params=variables)
    return out


def conformer_block(inputs, sequence_length, num_heads, ff_units, conv_kernel, keep=1.0, scope=None, attention_keep=1.0,
                    attention_window=None):
    """One Conformer block (Gulati et al. 2020; pre-norm, ESPnet's order) as ONE tape node:
        h = h + 1/2 drop(swish(LN(h) W1 + b1) W2 + b2)                   ffn1
        h = h + drop(self_attn(LN(h) Wqkv + b) Wo + bo)                  attention
        h = h + drop(conv_module(LN(h) Wp1 + bp1) Wp2 + bp2)             conv   (Wp1: D -> 2D, Wp2: D -> D)
        h = h + 1/2 drop(swish(LN(h) W3 + b3) W4 + b4)                   ffn2
        h = LN(h)                                                        out
    conv_module (conv_module.hip) is GLU, a depthwise convolution of `conv_kernel` taps along time, a layer norm per frame
    and Swish, over the frames < sequence_length of each row; its norm is a layer norm, not the paper's batch norm (the
    README says why).  inputs [B,T,D] fp32, D a multiple of 64.  The products run at GEMM_PRECISION, the attention at
    ATTENTION_PRECISION (exact fp32 by default), the convolution module is exact fp32.  keep: dropout keep probability (four draws per block under a tape).
    attention_keep: keep probability of the dropout on the attention probabilities, as in self_attention_block (one more
    draw under a tape when below 1, after the four).  attention_window: as in self_attention_block; it limits the attention
    only, the convolution module still reads (conv_kernel - 1) / 2 frames ahead.  Frames past a length carry finite values that no valid frame reads; the encoder masks them.
    Variables: <scope>/{ln_ff1,ln_att,ln_conv,ln_ff2,ln_out}/{gamma,beta}, ffn1/{fc1,fc2}/{weights,biases},
    attention/{qkv,out}/..., conv/{pw1,pw2}/..., conv/dw/{kernel [K,D],bias}, conv/norm/{gamma,beta}, ffn2/{fc1,fc2}/..."""
    lens = SeqLen.wrap(sequence_length, inputs.device)
    B, T, D = inputs.shape
    H, FF, K, N = int(num_heads), int(ff_units), int(conv_kernel), B * T
    if D % H or D // H not in (32, 64):
        raise ValueError('conformer_block: %d units in %d heads; the head width must be 32 or 64' % (D, H))
    if D % 64 or D > 1024 or K % 2 == 0 or not 3 <= K <= 31:
        raise ValueError('conformer_block: %d units and conv_kernel = %d; the convolution module takes a multiple of 64 '
                         'units up to 1024 and an odd kernel in 3..31' % (D, K))
    with vs.variable_scope(scope or 'conformer_block'):
        norms = [(vs.get_variable('%s/gamma' % n, [D], initializer=vs.ones), vs.get_variable('%s/beta' % n, [D], initializer=vs.zeros))
                 for n in ('ln_ff1', 'ln_att', 'ln_conv', 'ln_ff2', 'ln_out', 'conv/norm')]
        dense = [(vs.get_variable('%s/weights' % n, [i, o]), vs.get_variable('%s/biases' % n, [o], initializer=vs.zeros))
                 for n, i, o in (('ffn1/fc1', D, FF), ('ffn1/fc2', FF, D), ('attention/qkv', D, 3 * D), ('attention/out', D, D),
                                 ('conv/pw1', D, 2 * D), ('conv/pw2', D, D), ('ffn2/fc1', D, FF), ('ffn2/fc2', FF, D))]
        taps = vs.get_variable('conv/dw/kernel', [K, D])
        tap_bias = vs.get_variable('conv/dw/bias', [D], initializer=vs.zeros)
    variables = tuple(v for pair in norms + dense for v in pair) + (taps, tap_bias)
    cg, cb = norms[5]
    precision, attn_precision = GEMM_PRECISION[0], ATTENTION_PRECISION[0]
    training = Tape.current is not None
    rng = [ops.global_rng().next() for _ in range(4)] if training and keep < 1 else None
    attn_rng = ops.global_rng().next() if training and attention_keep < 1 else None

    def linear(x, i, width):
        W, b = dense[i]
        return hip.gemm(x, W.data, torch.empty((N, width), dtype=torch.float32, device=x.device), bias=b.data, precision=precision)

    def drop(x, i):
        return hip.dropout(x, keep, *rng[i]) if rng else x

    def norm(x, i):
        return hip.layer_norm_fwd(x, norms[i][0].data, norms[i][1].data, LN_EPS)

    def ffn(h, ni, di, ri):
        """(h + 1/2 drop(swish(LN(h) Wa + ba) Wb + bb), what its backward pass needs)"""
        a, mean, rstd = norm(h, ni)
        p = linear(a, di, FF)
        s = hip.swish(p)
        return hip.axpy_(h.clone(), drop(linear(s, di + 1, D), ri), a=0.5), (h, a, mean, rstd, p, s)

    x = (inputs if inputs.is_contiguous() else inputs.contiguous()).view(N, D)
    h1, ffn1 = ffn(x, 0, 0, 0)
    a2, mean2, rstd2 = norm(h1, 1)
    qkv = linear(a2, 2, 3 * D).view(B, T, 3 * D)
    c, lse = hip.self_attn_fwd(qkv, lens.dev, H, attn_precision, attention_keep, attn_rng, attention_window)
    h2 = hip.axpy_(drop(linear(c.view(N, D), 3, D), 1), h1)
    a3, mean3, rstd3 = norm(h2, 2)
    u = linear(a3, 4, 2 * D).view(B, T, 2 * D)
    v, cmean, crstd = hip.conv_module_fwd(u, lens.dev, taps.data, tap_bias.data, cg.data, cb.data, LN_EPS)
    h3 = hip.axpy_(drop(linear(v.view(N, D), 5, D), 2), h2)
    h4, ffn2 = ffn(h3, 3, 6, 3)
    out, mean5, rstd5 = norm(h4, 4)
    out = out.view(B, T, D)
    need_dx = requires_grad(inputs)

    def backward(dout):
        for var in variables:
            if var.grad is None:
                var.grad = torch.zeros_like(var.data)

        def linear_bwd(x, dy, i):
            """gradients of dense[i] (overwritten) at input x; returns dx"""
            W, b = dense[i]
            hip.gemm(x, dy, W.grad, trans_a=True, precision=precision)
            hip.colsum(dy, b.grad)
            return hip.gemm(dy, W.data, torch.empty_like(x), trans_b=True, precision=precision)

        def norm_bwd(x, dy, i, mean, rstd):
            dx, dgp, dbp = hip.layer_norm_bwd(x, norms[i][0].data, dy, mean, rstd)
            hip.colsum(dgp, norms[i][0].grad)
            hip.colsum(dbp, norms[i][1].grad)
            return dx

        def ffn_bwd(dh, kept, ni, di, ri):
            """dh at the sublayer's output -> dh at its input"""
            h, a, mean, rstd, p, s = kept
            half = hip.axpy_(torch.zeros_like(dh), drop(dh, ri), a=0.5)
            dp = hip.swish_bwd(p, linear_bwd(s, half, di + 1))
            return hip.axpy_(norm_bwd(h, linear_bwd(a, dp, di), ni, mean, rstd), dh)
        dh4 = norm_bwd(h4, dout.reshape(N, D).contiguous(), 4, mean5, rstd5)
        dh3 = ffn_bwd(dh4, ffn2, 3, 6, 3)
        dv = linear_bwd(v.view(N, D), drop(dh3, 2), 5)
        du, dw, dbw, dg, db = hip.conv_module_bwd(u, lens.dev, taps.data, tap_bias.data, cg.data, cb.data, cmean, crstd,
                                                  dv.view(B, T, D))
        for var, g in ((taps, dw), (tap_bias, dbw), (cg, dg), (cb, db)):
            var.grad.copy_(g)
        dh2 = hip.axpy_(norm_bwd(h2, linear_bwd(a3, du.reshape(N, 2 * D), 4), 2, mean3, rstd3), dh3)
        dc = linear_bwd(c.view(N, D), drop(dh2, 1), 3)
        dqkv = hip.self_attn_bwd(qkv, c, lse, dc.view(B, T, D), lens.dev, H, attn_precision, attention_keep, attn_rng,
                                 attention_window)
        dh1 = hip.axpy_(norm_bwd(h1, linear_bwd(a2, dqkv.reshape(N, 3 * D), 2), 1, mean2, rstd2), dh2)
        dx = ffn_bwd(dh1, ffn1, 0, 0, 0)                 # (the sublayer's own gradients are due either way)
        return [dx.view(B, T, D) if need_dx else None]
    record([inputs], [out], backward, params=variables)
    return out


def pblstm(inputs, sequence_length, num_units, num_steps=2, layer_norm=False, scope=None):
    """A pyramidal BLSTM layer (reference layer.py:53-94): blstm, then stack
    ``num_steps`` consecutive output frames.  Returns (outputs, new lengths)."""
    with vs.variable_scope(scope or 'PBLSTM'):
        outputs = blstm(inputs=inputs, sequence_length=sequence_length, num_units=num_units,
                        layer_norm=layer_norm, out_stack=num_steps if num_steps in (1, 2) else 0)
        outputs, output_seq_lengths = ops.pyramid_stack(outputs, sequence_length, num_steps)
    return outputs, output_seq_lengths
