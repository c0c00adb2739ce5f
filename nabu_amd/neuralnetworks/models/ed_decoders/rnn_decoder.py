"""General recurrent decoder (reference: models/ed_decoders/rnn_decoder.py:13-127).

``_decode`` keeps the reference's structure — pad the targets with the start
label C-1, build the cell, run it over the whole target sequence — but
``tf.contrib.seq2seq.dynamic_decode`` over a ScheduledEmbeddingTrainingHelper is
``dynamic_decode`` below: ONE call into the C ABI (nabu_speller_fwd) whose C++
driver launches, per decoder step, the recurrent GEMMs, the fused LSTM-cell
kernel, the query GEMM and the fused attention kernel (plus, with sample_prob > 0,
the step's projection and the scheduled-sampling kernel), and one output-projection
GEMM for all steps at the end.  Its gradient (nabu_speller_bwd) is the mirrored
loop with hand-written backward kernels; weight gradients that are sums over
steps are single GEMMs over all steps."""
import ctypes
from abc import ABCMeta, abstractmethod

import torch

from nabu_amd import _hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, SeqLen
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder


def _grad(var):
    if var.grad is None:
        var.grad = torch.zeros_like(var.data)
    return var.grad


def _ptrs(named, lstm, grad):
    """fill a nabu_speller_params / nabu_speller_grads struct"""
    s = _hip.SpellerPtrs()
    for k, var in named.items():
        setattr(s, k, None if var is None else _hip.ptr(_grad(var) if grad else var.data))
    for n, (kern, bias) in enumerate(lstm):
        s.lstm_kernel[n] = _hip.ptr(_grad(kern) if grad else kern.data)
        s.lstm_bias[n] = _hip.ptr(_grad(bias) if grad else bias.data)
    return s


def _ptrs_multi(named, lstm, grad):
    """fill a nabu_speller_multi_params / nabu_speller_multi_grads struct (per-mechanism lists in `named`)"""
    s = _hip.SpellerMultiPtrs()
    for k, var in named.items():
        if isinstance(var, list):
            arr = getattr(s, k)
            for m, v in enumerate(var):
                arr[m] = None if v is None else _hip.ptr(_grad(v) if grad else v.data)
        else:
            setattr(s, k, _hip.ptr(_grad(var) if grad else var.data))
    for n, (kern, bias) in enumerate(lstm):
        s.lstm_kernel[n] = _hip.ptr(_grad(kern) if grad else kern.data)
        s.lstm_bias[n] = _hip.ptr(_grad(bias) if grad else bias.data)
    return s


def cell_parameters(cell, E):
    """The variables of a projected attention cell (created on first use in the current scope,
    TF-style names) in the form the C ABI takes them.  Returns (attention mechanism, LSTM cells,
    number of layers, num_units, output dim, {name: Variable}, [(kernel, bias) per layer]).
    E: the encoder dimension, or a list of them for a cell over several memories — then the first item returned
    is the list of mechanisms and the per-mechanism entries of the dict are lists (mechanism order)."""
    wrapper = cell._cell
    if isinstance(E, (list, tuple)):
        return _cell_parameters_multi(cell, list(E))
    if len(wrapper.attention_mechanisms) != 1:
        raise ValueError('a cell over %d memories needs the list of their dimensions' % len(wrapper.attention_mechanisms))
    mech = wrapper.attention_mechanism
    cells = wrapper.cells
    nl = len(cells)
    U = cells[0].num_units
    if any(c.num_units != U for c in cells):
        raise NotImplementedError('all speller layers must have the same num_units')
    if nl > _hip.SPELLER_MAX_LAYERS:
        raise NotImplementedError('at most %d speller layers' % _hip.SPELLER_MAX_LAYERS)
    C = cell.output_size
    with vs.variable_scope('decoder'):
        av = mech.variables()
        with vs.variable_scope('attention_wrapper'):
            lstm = [c.variables(n, (C + E) if n == 0 else U) for n, c in enumerate(cells)]
        Wout, bout = cell.variables(E)
    named = dict(memory_kernel=av['memory_kernel'], query_kernel=av['query_kernel'],
                 attention_v=av['attention_v'], conv_kernel=av.get('conv_kernel'),
                 conv_proj=av.get('conv_proj'), out_kernel=Wout, out_bias=bout)
    return mech, cells, nl, U, C, named, lstm


def _cell_parameters_multi(cell, Es):
    wrapper = cell._cell
    mechs = wrapper.attention_mechanisms
    if len(mechs) != len(Es):
        raise ValueError('%d attention mechanisms, %d memories' % (len(mechs), len(Es)))
    if len(mechs) > _hip.SPELLER_MAX_MEMORIES:
        raise NotImplementedError('at most %d encoded inputs' % _hip.SPELLER_MAX_MEMORIES)
    cells = wrapper.cells
    nl = len(cells)
    U = cells[0].num_units
    if any(c.num_units != U for c in cells):
        raise NotImplementedError('all speller layers must have the same num_units')
    if nl > _hip.SPELLER_MAX_LAYERS:
        raise NotImplementedError('at most %d speller layers' % _hip.SPELLER_MAX_LAYERS)
    C = cell.output_size
    SE = sum(Es)
    with vs.variable_scope('decoder'):
        avs = [m.variables() for m in mechs]
        with vs.variable_scope('attention_wrapper'):
            lstm = [c.variables(n, (C + SE) if n == 0 else U) for n, c in enumerate(cells)]
        Wout, bout = cell.variables(SE)
    named = dict(out_kernel=Wout, out_bias=bout)
    for k in ('memory_kernel', 'query_kernel', 'attention_v', 'conv_kernel', 'conv_proj'):
        named[k] = [av.get(k) for av in avs]
    return mechs, cells, nl, U, C, named, lstm


def _dynamic_decode_multi(cell, encoded, encoded_seq_length, targets, target_seq_length, sample_prob):
    """dynamic_decode over M > 1 memories: ONE call into nabu_speller_multi_fwd (a step's M attention mechanisms are
    one launch); the tape node has M inputs and returns M dvalues"""
    dev = encoded[0].device
    M = len(encoded)
    B = encoded[0].shape[0]
    Tes, Es = [int(e.shape[1]) for e in encoded], [int(e.shape[2]) for e in encoded]
    mechs, cells, nl, U, C, named, lstm = cell_parameters(cell, Es)
    mech = mechs[0]
    tlen = SeqLen.wrap(target_seq_length, dev)
    elens = [SeqLen.wrap(l, dev) for l in encoded_seq_length]
    L = tlen.max()
    # the same draws as the one-memory decoder: neither the dropout masks nor the sampling depend on M
    keep = cells[0].output_keep_prob
    seed, offset = nops.global_rng().next() if keep < 1 else (0, 0)
    if keep < 1:
        nops.global_rng().offset += L * nl
    sprob = float(sample_prob)
    sseed, soffset = nops.global_rng().next() if sprob > 0 else (0, 0)
    if sprob > 0:
        nops.global_rng().offset += L
    i4 = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES
    desc = _hip.SpellerMultiDesc(ctypes.sizeof(_hip.SpellerMultiDesc), M, B, U, C, L, nl,
                                 i4(*(Tes + [0] * (_hip.SPELLER_MAX_MEMORIES - M))),
                                 i4(*(Es + [0] * (_hip.SPELLER_MAX_MEMORIES - M))), mech.kind, mech.filtersize,
                                 mech.numfilt, mech.prob_fn, keep, seed, offset * 1000003, sprob, sseed,
                                 soffset * 1000003)
    lib = _hip.lib()
    reserve_bytes = lib.nabu_speller_multi_reserve_bytes(ctypes.byref(desc))
    ws_bytes = lib.nabu_speller_multi_ws_bytes(ctypes.byref(desc))
    if reserve_bytes == 0:
        raise _hip.NabuHipError('speller: unsupported shape: %s' % lib.nabu_last_error().decode())
    ids = torch.full((L, B), C - 1, dtype=torch.int32, device=dev)
    if L > 1:
        ids[1:] = targets.to(torch.int32)[:, :L - 1].t()
    values = [e if e.is_contiguous() else e.contiguous() for e in encoded]
    vp = ctypes.c_void_p * M
    vals_p = vp(*[_hip.ptr(v) for v in values])
    elen_p = vp(*[_hip.ptr(l.dev) for l in elens])
    logits = torch.empty((B, L, C), dtype=torch.float32, device=dev)
    reserve = torch.empty(reserve_bytes, dtype=torch.uint8, device=dev)
    ws = _hip.Workspace.get(ws_bytes, dev, 'speller_multi')
    params = _ptrs_multi(named, lstm, grad=False)
    ev = dynamic_decode.events
    shape = dict(B=B, Te=Tes, E=Es, U=U, C=C, L=L)
    if ev is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _hip.check(lib.nabu_speller_multi_fwd(ctypes.byref(desc), vals_p, elen_p, _hip.ptr(ids), _hip.ptr(tlen.dev),
                                          ctypes.byref(params), _hip.ptr(logits), _hip.ptr(reserve), _hip.ptr(ws),
                                          ws_bytes, _hip.stream()), 'nabu_speller_multi_fwd')
    if ev is not None:
        e1.record()
        ev.append(('fwd', shape, e0, e1))

    def backward(dlogits):
        grads = _ptrs_multi(named, lstm, grad=True)
        p2 = _ptrs_multi(named, lstm, grad=False)
        dvalues = [torch.empty_like(v) for v in values]
        dv_p = vp(*[_hip.ptr(v) for v in dvalues])
        # (built here from the tensors themselves: the closure keeps the length vectors and the memories alive)
        vals_b, elen_b = vp(*[_hip.ptr(v) for v in values]), vp(*[_hip.ptr(l.dev) for l in elens])
        w2 = _hip.Workspace.get(ws_bytes, dev, 'speller_multi')
        evb = dynamic_decode.events
        if evb is not None:
            b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b0.record()
        _hip.check(lib.nabu_speller_multi_bwd(ctypes.byref(desc), vals_b, elen_b, _hip.ptr(ids), _hip.ptr(tlen.dev),
                                              ctypes.byref(p2), _hip.ptr(dlogits.contiguous()), _hip.ptr(reserve),
                                              ctypes.byref(grads), dv_p, _hip.ptr(w2), ws_bytes, _hip.stream()),
                   'nabu_speller_multi_bwd')
        if evb is not None:
            b1.record()
            evb.append(('bwd', shape, b0, b1))
        return dvalues

    record(list(encoded), [logits], backward)
    dynamic_decode.last = (desc, reserve)
    dynamic_decode.last_paths = (lib.nabu_speller_multi_uses_persistent(ctypes.byref(desc), 0),
                                 lib.nabu_speller_multi_uses_persistent(ctypes.byref(desc), 1))
    return logits, tlen


def dynamic_decode(cell, encoded, encoded_seq_length, targets, target_seq_length, sample_prob,
                   is_training):  # noqa: C901
    """Run the projected attention cell over the target sequence.

    encoded [B,Te,E] (rows >= length zero), targets [B,Lt] int32 (already holding EOS
    where the recipe uses it), target_seq_length [B].  Returns logits [B,L,C] with
    L = max(target_seq_length); rows of finished utterances are zero.
    encoded / encoded_seq_length may be lists (one entry per attention mechanism of the cell): one memory takes
    the one-memory entry points below, several take nabu_speller_multi_*."""
    if isinstance(encoded, (list, tuple)):
        if len(encoded) != 1:
            return _dynamic_decode_multi(cell, list(encoded), list(encoded_seq_length), targets, target_seq_length,
                                         sample_prob)
        encoded, encoded_seq_length = encoded[0], encoded_seq_length[0]
    dev = encoded.device
    B, Te, E = encoded.shape
    mech, cells, nl, U, C, named, lstm = cell_parameters(cell, E)
    tlen = SeqLen.wrap(target_seq_length, dev)
    elen = SeqLen.wrap(encoded_seq_length, dev)
    L = tlen.max()

    keep = cells[0].output_keep_prob
    seed, offset = nops.global_rng().next() if keep < 1 else (0, 0)
    if keep < 1:
        nops.global_rng().offset += L * nl          # one mask per (step, layer)
    # scheduled sampling (ScheduledEmbeddingTrainingHelper, rnn_decoder.py:59-66); like the
    # reference it is active whenever _decode runs, in the training and the validation graph
    sprob = float(sample_prob)
    sseed, soffset = nops.global_rng().next() if sprob > 0 else (0, 0)
    if sprob > 0:
        nops.global_rng().offset += L
    desc = _hip.SpellerDesc(ctypes.sizeof(_hip.SpellerDesc), B, Te, E, U, C, L, nl, mech.kind,
                            mech.filtersize, mech.numfilt, mech.prob_fn, keep, seed, offset * 1000003,
                            sprob, sseed, soffset * 1000003)
    lib = _hip.lib()
    reserve_bytes = lib.nabu_speller_reserve_bytes(ctypes.byref(desc))
    ws_bytes = lib.nabu_speller_ws_bytes(ctypes.byref(desc))
    if reserve_bytes == 0:
        raise _hip.NabuHipError('speller: unsupported shape: %s' % lib.nabu_last_error().decode())

    # decoder inputs: [SOS = C-1, y_0 .. y_{L-2}] (rnn_decoder.py:46-47), time-major ids
    ids = torch.full((L, B), C - 1, dtype=torch.int32, device=dev)
    if L > 1:
        ids[1:] = targets.to(torch.int32)[:, :L - 1].t()
    values = encoded if encoded.is_contiguous() else encoded.contiguous()
    logits = torch.empty((B, L, C), dtype=torch.float32, device=dev)
    reserve = torch.empty(reserve_bytes, dtype=torch.uint8, device=dev)
    ws = _hip.Workspace.get(ws_bytes, dev, 'speller')
    params = _ptrs(named, lstm, grad=False)
    ev = dynamic_decode.events          # (bench.py: a list while a step's decoder calls are to be bracketed by events)
    shape = dict(B=B, Te=Te, E=E, U=U, C=C, L=L)
    if ev is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _hip.check(lib.nabu_speller_fwd(ctypes.byref(desc), _hip.ptr(values), _hip.ptr(elen.dev), _hip.ptr(ids),
                                    _hip.ptr(tlen.dev), ctypes.byref(params), _hip.ptr(logits),
                                    _hip.ptr(reserve), _hip.ptr(ws), ws_bytes, _hip.stream()),
               'nabu_speller_fwd')
    if ev is not None:
        e1.record()
        ev.append(('fwd', shape, e0, e1))

    def backward(dlogits):
        grads = _ptrs(named, lstm, grad=True)
        p2 = _ptrs(named, lstm, grad=False)
        dvalues = torch.empty_like(values)
        w2 = _hip.Workspace.get(ws_bytes, dev, 'speller')
        evb = dynamic_decode.events
        if evb is not None:
            b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b0.record()
        _hip.check(lib.nabu_speller_bwd(ctypes.byref(desc), _hip.ptr(values), _hip.ptr(elen.dev),
                                        _hip.ptr(ids), _hip.ptr(tlen.dev), ctypes.byref(p2),
                                        _hip.ptr(dlogits.contiguous()), _hip.ptr(reserve),
                                        ctypes.byref(grads), _hip.ptr(dvalues), _hip.ptr(w2), ws_bytes,
                                        _hip.stream()), 'nabu_speller_bwd')
        if evb is not None:
            b1.record()
            evb.append(('bwd', shape, b0, b1))
        return [dvalues]

    record([encoded], [logits], backward)
    dynamic_decode.last = (desc, reserve)           # for decoder_inputs() below (tests, diagnostics)
    dynamic_decode.last_paths = (lib.nabu_speller_uses_persistent(ctypes.byref(desc), 0),
                                 lib.nabu_speller_uses_persistent(ctypes.byref(desc), 1))
    return logits, tlen



dynamic_decode.events = None


def beam_search(cell, encoded, encoded_seq_length, beam_width, max_steps, length_penalty=0.0,
                temperature=1.0, with_alignments=True):
    """Beam search over the projected attention cell (components/beam_search_decoder.py:68-451
    under dynamic_decode): ONE call into the C ABI (nabu_speller_beam_search), whose C++ driver runs
    the cell kernels on B*beam_width rows, prunes and gathers on the device, and stops as the
    reference's dynamic_decode does.  encoded [B,Te,E] (rows >= length zero).
    Returns (sequences [B,W,time] int32, lengths [B,W] int32, scores [B,W], alignments
    [B,W,time,Te] or None).  encoded / encoded_seq_length may be lists (one entry per attention mechanism): several
    memories run nabu_speller_multi_beam_search and return the alignments as a list of [B,W,time,Te_m], one per memory."""
    if isinstance(encoded, (list, tuple)):
        if len(encoded) != 1:
            return _beam_search_multi(cell, list(encoded), list(encoded_seq_length), beam_width, max_steps,
                                      length_penalty, temperature, with_alignments)
        encoded, encoded_seq_length = encoded[0], encoded_seq_length[0]
    dev = encoded.device
    B, Te, E = encoded.shape
    mech, cells, nl, U, C, named, lstm = cell_parameters(cell, E)
    elen = SeqLen.wrap(encoded_seq_length, dev)
    W, S = int(beam_width), int(max_steps)
    desc = _hip.BeamDesc(ctypes.sizeof(_hip.BeamDesc), B, Te, E, U, C, nl, mech.kind, mech.filtersize,
                         mech.numfilt, mech.prob_fn, W, S, float(length_penalty), float(temperature))
    lib = _hip.lib()
    ws_bytes = lib.nabu_speller_beam_ws_bytes(ctypes.byref(desc))
    if ws_bytes == 0:
        raise _hip.NabuHipError('beam search: unsupported shape: %s' % lib.nabu_last_error().decode())
    values = encoded if encoded.is_contiguous() else encoded.contiguous()
    seq = torch.empty((B, W, S), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    align = torch.empty((B, W, S, Te), dtype=torch.float32, device=dev) if with_alignments else None
    ws = _hip.Workspace.get(ws_bytes, dev, 'beam_search')
    params = _ptrs(named, lstm, grad=False)
    steps = ctypes.c_int32(0)
    _hip.check(lib.nabu_speller_beam_search(ctypes.byref(desc), _hip.ptr(values), _hip.ptr(elen.dev),
                                            ctypes.byref(params), _hip.ptr(seq), _hip.ptr(lengths),
                                            _hip.ptr(scores), _hip.ptr(align), ctypes.byref(steps),
                                            _hip.ptr(ws), ws_bytes, _hip.stream()), 'nabu_speller_beam_search')
    n = steps.value
    return seq[:, :, :n], lengths, scores, (align[:, :, :n] if with_alignments else None)

def _beam_search_multi(cell, encoded, encoded_seq_length, beam_width, max_steps, length_penalty, temperature,
                       with_alignments):
    dev = encoded[0].device
    M, B = len(encoded), encoded[0].shape[0]
    Tes, Es = [int(e.shape[1]) for e in encoded], [int(e.shape[2]) for e in encoded]
    mechs, cells, nl, U, C, named, lstm = cell_parameters(cell, Es)
    mech = mechs[0]
    elens = [SeqLen.wrap(l, dev) for l in encoded_seq_length]
    W, S = int(beam_width), int(max_steps)
    i4 = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES
    pad = [0] * (_hip.SPELLER_MAX_MEMORIES - M)
    desc = _hip.MultiBeamDesc(ctypes.sizeof(_hip.MultiBeamDesc), M, B, U, C, nl, i4(*(Tes + pad)), i4(*(Es + pad)),
                              mech.kind, mech.filtersize, mech.numfilt, mech.prob_fn, W, S, float(length_penalty),
                              float(temperature))
    lib = _hip.lib()
    ws_bytes = lib.nabu_speller_multi_beam_ws_bytes(ctypes.byref(desc))
    if ws_bytes == 0:
        raise _hip.NabuHipError('beam search: unsupported shape: %s' % lib.nabu_last_error().decode())
    values = [e if e.is_contiguous() else e.contiguous() for e in encoded]
    vp = ctypes.c_void_p * M
    seq = torch.empty((B, W, S), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    aligns = [torch.empty((B, W, S, Te), dtype=torch.float32, device=dev) for Te in Tes] if with_alignments else None
    ws = _hip.Workspace.get(ws_bytes, dev, 'beam_search_multi')
    params = _ptrs_multi(named, lstm, grad=False)
    steps = ctypes.c_int32(0)
    _hip.check(lib.nabu_speller_multi_beam_search(
        ctypes.byref(desc), vp(*[_hip.ptr(v) for v in values]), vp(*[_hip.ptr(l.dev) for l in elens]),
        ctypes.byref(params), _hip.ptr(seq), _hip.ptr(lengths), _hip.ptr(scores),
        vp(*[_hip.ptr(a) for a in aligns]) if with_alignments else None, ctypes.byref(steps), _hip.ptr(ws), ws_bytes,
        _hip.stream()), 'nabu_speller_multi_beam_search')
    n = steps.value
    return seq[:, :, :n], lengths, scores, ([a[:, :, :n] for a in aligns] if with_alignments else None)


def decoder_inputs():
    """[L,B] int32 labels the last dynamic_decode fed to the cell (row 0 = SOS; later rows are the
    targets shifted by one, or samples where scheduled sampling replaced them)"""
    desc, reserve = dynamic_decode.last
    out = torch.empty((desc.L, desc.B), dtype=torch.int32, device=reserve.device)
    multi = isinstance(desc, _hip.SpellerMultiDesc)
    fn = _hip.lib().nabu_speller_multi_decoder_inputs if multi else _hip.lib().nabu_speller_decoder_inputs
    _hip.check(fn(ctypes.byref(desc), _hip.ptr(reserve), _hip.ptr(out), _hip.stream()),
               'nabu_speller_multi_decoder_inputs' if multi else 'nabu_speller_decoder_inputs')
    return out


class RNNDecoder(ed_decoder.EDDecoder, metaclass=ABCMeta):
    '''a recurrent decoder: _decode runs the cell built by create_cell over the targets'''

    def _decode(self, encoded, encoded_seq_length, targets, target_seq_length, is_training):
        # only the first target / output is used (rnn_decoder.py:40-47)
        tname = list(targets.keys())[0]
        output_name = list(self.output_dims.keys())[0]
        rnn_cell = self.create_cell(encoded, encoded_seq_length, is_training)
        # every encoded input, in the order of `encoded` (the order of the cell's attention mechanisms)
        enames = list(encoded.keys())
        logits, logit_seq_length = dynamic_decode(
            rnn_cell, [encoded[e] for e in enames], [encoded_seq_length[e] for e in enames], targets[tname],
            target_seq_length[tname], float(self.conf['sample_prob']), is_training)
        return {output_name: logits}, {output_name: logit_seq_length}, ()

    @abstractmethod
    def create_cell(self, encoded, encoded_seq_length, is_training):
        '''create the rnn cell'''

    def zero_state(self, encoded_dim, batch_size):
        '''the decoder zero state: zero cell/hidden states, context and alignments'''
        return ()
