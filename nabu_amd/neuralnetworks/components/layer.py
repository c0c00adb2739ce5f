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


def pblstm(inputs, sequence_length, num_units, num_steps=2, layer_norm=False, scope=None):
    """A pyramidal BLSTM layer (reference layer.py:53-94): blstm, then stack
    ``num_steps`` consecutive output frames.  Returns (outputs, new lengths)."""
    with vs.variable_scope(scope or 'PBLSTM'):
        outputs = blstm(inputs=inputs, sequence_length=sequence_length, num_units=num_units,
                        layer_norm=layer_norm, out_stack=num_steps if num_steps in (1, 2) else 0)
        outputs, output_seq_lengths = ops.pyramid_stack(outputs, sequence_length, num_steps)
    return outputs, output_seq_lengths
