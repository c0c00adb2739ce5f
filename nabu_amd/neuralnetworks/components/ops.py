"""Tensor plumbing ops of the hot path (reference: nabu/neuralnetworks/components/ops.py)."""
import weakref

import numpy as np

from nabu_amd import ops as hip
from nabu_amd.autodiff import record, requires_grad, SeqLen


# A-priori magnitude bound of a tensor on the path, an attribute of the tensor OBJECT: layer.blstm records |out| <= 1
# (o tanh c), the plumbing ops below carry the bound along, and the next layer hands it to the C ABI
# (nabu_blstm_desc.x_bound), whose f16x3 operand packs then take their row scales from it instead of measuring x.
# The bound is a promise: tensors that carry one must not be modified in place (a stale bound makes the f16x3 packs
# overflow fp16 silently).  NABU_CHECK_X_BOUND=1 (layer.CHECK_X_BOUND) measures and asserts at every layer.
def set_value_bound(tensor, bound):
    tensor._nabu_value_bound = float(bound)


def value_bound(tensor):
    """the recorded bound on |tensor|, 0.0 when nothing is known"""
    return getattr(tensor, '_nabu_value_bound', 0.0)


# PACKED COMPANION of a tensor on the path (include/nabu_hip.h, nabu_blstm_desc ABI version 3), an attribute of the
# tensor object like its bound: layer.blstm asks the forward recurrent kernel to write its output ALSO as the next
# layer's f16x3 operands (rows, cols) for the frame stacking `stack` that pyramid_stack is about to apply, and the next
# layer.blstm hands them to the C ABI instead of packing its input.  Only the stacking view carries a companion along;
# any op that makes a new tensor (dropout, noise) drops it, and the next layer packs for itself as before.
def set_packed(tensor, stack, bufs):
    tensor._nabu_packed = (int(stack), bufs)


def packed(tensor, stack):
    """the (rows, cols) companion of `tensor` written for frame stacking `stack`, or None"""
    e = getattr(tensor, '_nabu_packed', None)
    return e[1] if e is not None and e[0] == stack else None


class BufferPool(object):
    """Zero-filled uint8 device buffers reused call after call by one user, key = (a layer's scope, role): a companion
    is rewritten in full by every forward call of one shape and its padding stays zero.  acquire() hands out a fresh
    view of a slot's buffer, and the slot stays busy exactly as long as that view object is alive: whoever still reads
    the buffer (a pending backward pass through its plan, a consumer's plan, an output carrying it as its packed()
    companion) holds the view itself, never a slice of it.  So at most (live holders + 1) buffers per key."""

    def __init__(self):
        self._slots = {}        # key -> [[buffer, layout, weak reference to the view handed out]]

    def acquire(self, key, nbytes, device, layout=()):
        """a buffer of `nbytes` zero-filled for `layout` (what, beside its size, decides which bytes a user writes):
        a free slot of the same size, device and layout, else a new one, after the free slots of `key` are freed"""
        import torch
        slots = self._slots.setdefault(key, [])
        for slot in slots:
            buf, lay, ref = slot
            if ref() is None and buf.numel() == nbytes and buf.device == torch.device(device) and lay == layout:
                view = buf.view(-1)
                slot[2] = weakref.ref(view)
                return view
        slots[:] = [s for s in slots if s[2]() is not None]
        buf = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
        view = buf.view(-1)
        slots.append([buf, layout, weakref.ref(view)])
        return view

    def held_bytes(self, role=None):
        """bytes held (busy or free) in the slots whose key ends in `role`, or in all of them"""
        return sum(s[0].numel() for key, slots in self._slots.items() if role is None or key[-1] == role for s in slots)


companions = BufferPool()


def pyramid_stack(inputs, sequence_lengths, numsteps, axis=2, scope=None):
    """Concatenate ``numsteps`` consecutive frames on the feature axis
    (reference ops.py:6-60).

    inputs [B,T,F] batch-major contiguous -> [B, ceil(T/numsteps), numsteps*F];
    lengths -> ceil(len/numsteps) (ops.py:56-58).  On a batch-major buffer the
    stack of consecutive frames IS a reshape, so for T % numsteps == 0 this is a
    free view; otherwise the time axis is zero-padded first (ops.py:32-38)."""
    if axis != 2:
        raise Exception('pyramid_stack: only axis=2 is supported')
    B, T, F = inputs.shape
    Tp = -(-T // numsteps) * numsteps
    src = inputs if Tp == T else hip.pad_time(inputs, Tp)
    outputs = src.view(B, Tp // numsteps, numsteps * F)
    if value_bound(inputs):
        set_value_bound(outputs, value_bound(inputs))
    if Tp == T and packed(inputs, numsteps) is not None:        # the companion was written for exactly this stacking
        set_packed(outputs, 1, packed(inputs, numsteps))

    def backward(dout):
        d = dout.reshape(B, Tp, F)
        return [d if Tp == T else hip.unpad_time(d, T)]
    record([inputs], [outputs], backward)
    lens = SeqLen.wrap(sequence_lengths)
    # (a length vector is immutable: the stacked lengths of a SeqLen OBJECT that comes round again — a batch kept on the
    # device, the layers of one step sharing it — are derived once)
    cache = lens.__dict__.setdefault('_stacked', {})
    if numsteps not in cache:
        new_host = -(-lens.host // numsteps)
        # the device copy is derived on the device: an upload here would block the host on the stream
        cache[numsteps] = SeqLen(new_host.astype(np.int32), dev_tensor=hip.ceil_div_i32(lens.dev, numsteps))
    return outputs, cache[numsteps]


def dense_sequence_to_sparse(sequences, sequence_lengths):
    """The reference converts dense targets to a tf.SparseTensor for tf.nn.ctc_loss
    (ops.py:121-145).  The HIP CTC kernel reads the dense [B,Lmax] labels plus the
    length vector directly, so this returns them unchanged (kept for API parity)."""
    return sequences, sequence_lengths


def seq_dropout(x, keep_prob, rng_state):
    """tf.nn.dropout(x, keep_prob) with a regenerable Philox mask."""
    seed, offset = rng_state.next()
    y = hip.dropout(x, keep_prob, seed, offset)
    if value_bound(x):
        set_value_bound(y, value_bound(x) / keep_prob)

    def backward(dy):
        return [hip.dropout(dy.contiguous(), keep_prob, seed, offset)]
    record([x], [y], backward)
    return y


def input_noise(x, stddev, rng_state):
    """inputs + tf.random_normal(shape, stddev) (listener.py:40-45)."""
    seed, offset = rng_state.next()
    y = hip.gaussian_noise(x, stddev, seed, offset)
    if requires_grad(x):     # (raw features: the noisy copy depends on no parameter either — the first layer then skips
        record([x], [y], lambda dy: [dy])   # its input gradient, two [B T, 8H] x [8H, D] products per step)
    return y


def spec_augment(x, lengths, policy, rng_state):
    """SpecAugment of the features x [B, T, D] (hip.SpecAugmentPolicy; the rules: DESIGN.md): a time warp about a random
    anchor frame, then time and frequency masks of zeros, drawn per utterance from ONE rng_state.next().  A policy
    that is off makes no call and consumes no offset."""
    if not policy.on:
        return x
    if requires_grad(x):     # (interpolation has a gradient, and nothing here computes it: features are leaves)
        raise Exception('spec_augment: the features depend on a parameter; the augmentation computes no input gradient')
    if x.shape[2] % policy.feature_blocks:
        raise ValueError('feature_blocks = %d does not divide the feature dimension %d' % (policy.feature_blocks,
                                                                                          x.shape[2]))
    lens = SeqLen.wrap(lengths, x.device)
    seed, offset = rng_state.next()
    y = hip.spec_augment(x if x.is_contiguous() else x.contiguous(), lens.dev, policy, seed, offset)
    if value_bound(x):       # (a convex combination of two frames, or zero: no larger than its inputs)
        set_value_bound(y, value_bound(x))
    return y


def tile_rows(x, R):
    """x [B, ...] repeated R times along the batch, replica-major: y[r * B + b] = x[b] (one encoder pass under several
    decoder rows: trainers/mwer.py).  The gradient is the sum over the replicas in the order r = 0..R-1.  Lengths are
    tiled on the host by the caller."""
    y = hip.rows_tile(x, R)
    if value_bound(x):
        set_value_bound(y, value_bound(x))
    if requires_grad(x):
        record([x], [y], lambda dy: [hip.rows_tile_bwd(dy, R)])
    return y


class RngState(object):
    """Seed + running offset for the counter-based device RNG."""

    def __init__(self, seed=0):
        self.seed = int(seed)
        self.offset = 0

    def next(self):
        self.offset += 1
        return self.seed, self.offset


_rng = RngState(0)


def global_rng():
    return _rng


def set_seed(seed):
    _rng.seed = int(seed)
    _rng.offset = 0
