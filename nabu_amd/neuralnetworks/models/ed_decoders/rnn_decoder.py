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


class _Binding(object):
    """What depends on which C entry points a call takes: nabu_speller_* (one memory; scalars and plain pointers) or
    nabu_speller_multi_* (M memories; Te / E arrays in the descriptor, host arrays of device pointers)."""

    def __init__(self, prefix, multi, ptrs_cls, desc_cls, beam_desc_cls, ws_key, beam_ws_key):
        self.prefix, self.multi, self.ptrs_cls = prefix, multi, ptrs_cls
        self.desc_cls, self.beam_desc_cls, self.ws_key, self.beam_ws_key = desc_cls, beam_desc_cls, ws_key, beam_ws_key

    def fn(self, name):
        """one of reserve_bytes, ws_bytes, uses_persistent, fwd, bwd, beam_ws_bytes, beam_search, sample_ws_bytes, sample"""
        return getattr(_hip.lib(), self.prefix + name)

    def desc(self, cls, Tes, Es, **fields):
        if self.multi:
            i4, pad = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES, [0] * (_hip.SPELLER_MAX_MEMORIES - len(Tes))
            fields.update(M=len(Tes), Te=i4(*(Tes + pad)), E=i4(*(Es + pad)))
        else:
            fields.update(Te=Tes[0], E=Es[0])
        return cls(size=ctypes.sizeof(cls), **fields)

    def per_memory(self, items):
        """a per-memory list as this binding's callers see it: the list, or its only item"""
        return items if self.multi else items[0]

    def pointers(self, tensors):
        """values / enc_len / dvalues / alignments: a host array of device pointers, or the pointer"""
        if tensors is None:
            return None
        if self.multi:
            return (ctypes.c_void_p * len(tensors))(*[_hip.ptr(t) for t in tensors])
        return _hip.ptr(tensors[0])

    def params(self, named, lstm, grad):
        """fill a nabu_speller[_multi]_params / _grads struct (per-mechanism entries of `named` are lists)"""
        s = self.ptrs_cls()
        p = lambda var: None if var is None else _hip.ptr(_grad(var) if grad else var.data)
        for k, var in named.items():
            if not isinstance(var, list):
                setattr(s, k, p(var))
            elif self.multi:
                for m, v in enumerate(var):
                    getattr(s, k)[m] = p(v)
            else:
                setattr(s, k, p(var[0]))
        for n, (kern, bias) in enumerate(lstm):
            s.lstm_kernel[n], s.lstm_bias[n] = p(kern), p(bias)
        return s


_ONE = _Binding('nabu_speller_', False, _hip.SpellerPtrs, _hip.SpellerDesc, _hip.BeamDesc, 'speller', 'beam_search')
_MULTI = _Binding('nabu_speller_multi_', True, _hip.SpellerMultiPtrs, _hip.SpellerMultiDesc, _hip.MultiBeamDesc,
                  'speller_multi', 'beam_search_multi')
_force_multi = False        # (tests: one memory through nabu_speller_multi_*, which the C side supports for M = 1)


def _memories(encoded, encoded_seq_length):
    """(binding, [encoded], [lengths]) of a tensor or a list of them: one memory takes nabu_speller_* (with the
    persistent decoder and the stream chain), several take nabu_speller_multi_*"""
    if not isinstance(encoded, (list, tuple)):
        encoded, encoded_seq_length = [encoded], [encoded_seq_length]
    return (_MULTI if len(encoded) > 1 or _force_multi else _ONE), list(encoded), list(encoded_seq_length)


def cell_parameters(cell, E):
    """The variables of a projected attention cell (created on first use in the current scope,
    TF-style names) in the form the C ABI takes them.  Returns (attention mechanism, LSTM cells,
    number of layers, num_units, output dim, {name: Variable}, [(kernel, bias) per layer]).
    E: the encoder dimension, or a list of them for a cell over several memories — then the first item returned
    is the list of mechanisms and the per-mechanism entries of the dict are lists (mechanism order)."""
    wrapper = cell._cell
    Es = list(E) if isinstance(E, (list, tuple)) else [E]
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
    if not isinstance(E, (list, tuple)):
        return mechs[0], cells, nl, U, C, {k: v[0] if isinstance(v, list) else v for k, v in named.items()}, lstm
    return mechs, cells, nl, U, C, named, lstm


def dynamic_decode(cell, encoded, encoded_seq_length, targets, target_seq_length, sample_prob,
                   is_training):  # noqa: C901
    """Run the projected attention cell over the target sequence.

    encoded [B,Te,E] (rows >= length zero), targets [B,Lt] int32 (already holding EOS
    where the recipe uses it), target_seq_length [B].  Returns logits [B,L,C] with
    L = max(target_seq_length); rows of finished utterances are zero.
    encoded / encoded_seq_length may be lists (one entry per attention mechanism of the cell); the tape node then
    has M inputs and returns M dvalues."""
    abi, encoded, encoded_seq_length = _memories(encoded, encoded_seq_length)
    dev = encoded[0].device
    B = encoded[0].shape[0]
    Tes, Es = [int(e.shape[1]) for e in encoded], [int(e.shape[2]) for e in encoded]
    mechs, cells, nl, U, C, named, lstm = cell_parameters(cell, Es)
    mech = mechs[0]
    tlen = SeqLen.wrap(target_seq_length, dev)
    elens = [SeqLen.wrap(l, dev) for l in encoded_seq_length]
    L = tlen.max()

    # neither the dropout masks nor the sampling depend on the number of memories
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
    desc = abi.desc(abi.desc_cls, Tes, Es, B=B, U=U, C=C, L=L, num_layers=nl, kind=mech.kind, K=mech.filtersize,
                    F=mech.numfilt, prob_fn=mech.prob_fn, keep_prob=keep, seed=seed, seed_offset=offset * 1000003,
                    sample_prob=sprob, sample_seed=sseed, sample_offset=soffset * 1000003)
    reserve_bytes = abi.fn('reserve_bytes')(ctypes.byref(desc))
    ws_bytes = abi.fn('ws_bytes')(ctypes.byref(desc))
    if reserve_bytes == 0:
        raise _hip.NabuHipError('speller: unsupported shape: %s' % _hip.lib().nabu_last_error().decode())

    # decoder inputs: [SOS = C-1, y_0 .. y_{L-2}] (rnn_decoder.py:46-47), time-major ids
    ids = torch.full((L, B), C - 1, dtype=torch.int32, device=dev)
    if L > 1:
        ids[1:] = targets.to(torch.int32)[:, :L - 1].t()
    values = [e if e.is_contiguous() else e.contiguous() for e in encoded]
    logits = torch.empty((B, L, C), dtype=torch.float32, device=dev)
    reserve = torch.empty(reserve_bytes, dtype=torch.uint8, device=dev)
    shape = dict(B=B, Te=abi.per_memory(Tes), E=abi.per_memory(Es), U=U, C=C, L=L)

    def call(which, *args):
        """one pass, bracketed by events while bench.py collects them (dynamic_decode.events is a list)"""
        ev = dynamic_decode.events
        # (the pointer arrays are built here from the tensors themselves: the closure keeps the length vectors and the
        #  memories alive)
        vals_p, elen_p = abi.pointers(values), abi.pointers([l.dev for l in elens])
        params, fn = abi.params(named, lstm, grad=False), abi.fn(which)
        ws = _hip.Workspace.get(ws_bytes, dev, abi.ws_key)
        if ev is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        _hip.check(fn(ctypes.byref(desc), vals_p, elen_p, _hip.ptr(ids), _hip.ptr(tlen.dev), ctypes.byref(params), *args,
                      _hip.ptr(ws), ws_bytes, _hip.stream()), abi.prefix + which)
        if ev is not None:
            e1.record()
            ev.append((which, shape, e0, e1))

    call('fwd', _hip.ptr(logits), _hip.ptr(reserve))

    def backward(dlogits):
        grads = abi.params(named, lstm, grad=True)
        dvalues = [torch.empty_like(v) for v in values]
        call('bwd', _hip.ptr(dlogits.contiguous()), _hip.ptr(reserve), ctypes.byref(grads), abi.pointers(dvalues))
        return dvalues

    record(encoded, [logits], backward)
    dynamic_decode.last = (desc, reserve)           # for decoder_inputs() below (tests, diagnostics)
    dynamic_decode.last_paths = (abi.fn('uses_persistent')(ctypes.byref(desc), 0),
                                 abi.fn('uses_persistent')(ctypes.byref(desc), 1))
    return logits, tlen


dynamic_decode.events = None


def _free_run(which, cell, encoded, encoded_seq_length, beam_width, max_steps, length_penalty, temperature,
              with_alignments, *extra):
    """The call beam_search and sample share: `which` is 'beam' (nabu_speller[_multi]_beam_search) or 'sample'
    (nabu_speller[_multi]_sample, beam_width 1, `extra` = seed, offset) or 'beam_joint'
    (nabu_speller[_multi]_beam_search_joint, `extra` = the CTC head's logits, ctc_weight) or 'beam_ex'
    (nabu_speller[_multi]_beam_search_ex, `extra` = a _hip.BeamSearchOpts).  Returns (sequences [B,W,time] int32,
    lengths [B,W] int32, scores or nll [B,W], [alignments [B,W,time,Te_m] per memory] or None, the binding)."""
    abi, encoded, encoded_seq_length = _memories(encoded, encoded_seq_length)
    dev = encoded[0].device
    B = encoded[0].shape[0]
    Tes, Es = [int(e.shape[1]) for e in encoded], [int(e.shape[2]) for e in encoded]
    mechs, cells, nl, U, C, named, lstm = cell_parameters(cell, Es)
    mech = mechs[0]
    elens = [SeqLen.wrap(l, dev) for l in encoded_seq_length]
    W, S = int(beam_width), int(max_steps)
    desc = abi.desc(abi.beam_desc_cls, Tes, Es, B=B, U=U, C=C, num_layers=nl, kind=mech.kind, K=mech.filtersize,
                    F=mech.numfilt, prob_fn=mech.prob_fn, beam_width=W, max_steps=S,
                    length_penalty=float(length_penalty), temperature=float(temperature))
    name = {'beam': 'beam_search', 'beam_joint': 'beam_search_joint', 'beam_ex': 'beam_search_ex'}.get(which, which)
    if which == 'beam_ex':          # the options decide the workspace, and go to the call by reference
        extra = (ctypes.byref(extra[0]),)
        ws_bytes = abi.fn(which + '_ws_bytes')(ctypes.byref(desc), extra[0])
    else:
        ws_bytes = abi.fn(which + '_ws_bytes')(ctypes.byref(desc))
    if ws_bytes == 0:
        raise _hip.NabuHipError('%s: unsupported shape: %s' % (name, _hip.lib().nabu_last_error().decode()))
    values = [e if e.is_contiguous() else e.contiguous() for e in encoded]
    seq = torch.empty((B, W, S), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, W), dtype=torch.int32, device=dev)
    scores = torch.empty((B, W), dtype=torch.float32, device=dev)
    aligns = [torch.empty((B, W, S, Te), dtype=torch.float32, device=dev) for Te in Tes] if with_alignments else None
    ws = _hip.Workspace.get(ws_bytes, dev, abi.beam_ws_key)
    params = abi.params(named, lstm, grad=False)
    steps = ctypes.c_int32(0)
    _hip.check(abi.fn(name)(ctypes.byref(desc), abi.pointers(values), abi.pointers([l.dev for l in elens]),
                            ctypes.byref(params), *extra, _hip.ptr(seq), _hip.ptr(lengths), _hip.ptr(scores),
                            abi.pointers(aligns), ctypes.byref(steps), _hip.ptr(ws), ws_bytes, _hip.stream()),
               abi.prefix + name)
    n = steps.value
    return seq[:, :, :n], lengths, scores, ([a[:, :, :n] for a in aligns] if with_alignments else None), abi


def beam_search(cell, encoded, encoded_seq_length, beam_width, max_steps, length_penalty=0.0,
                temperature=1.0, with_alignments=True, ctc_logits=None, ctc_weight=0.0, lm=None, lm_weight=0.0):
    """Beam search over the projected attention cell (components/beam_search_decoder.py:68-451
    under dynamic_decode): ONE call into the C ABI (nabu_speller_beam_search), whose C++ driver runs
    the cell kernels on B*beam_width rows, prunes and gathers on the device, and stops as the
    reference's dynamic_decode does.  encoded [B,Te,E] (rows >= length zero).
    Returns (sequences [B,W,time] int32, lengths [B,W] int32, scores [B,W], alignments
    [B,W,time,Te] or None).  encoded / encoded_seq_length may be lists (one entry per attention mechanism): several
    memories run nabu_speller_multi_beam_search and return the alignments as a list of [B,W,time,Te_m], one per memory.
    ctc_logits [B,Te,C] (the CTC head's logits on the FIRST encoded input) with ctc_weight in (0, 1): the joint
    CTC/attention search of nabu_speller[_multi]_beam_search_joint; without them the plain entry point is called.
    lm (a processing.ngram_lm.NgramLM over the cell's C symbols) with lm_weight > 0: shallow fusion, every candidate of a
    live beam adds lm_weight * log p_lm(label | the hypothesis' last n-1 labels) (nabu_speller[_multi]_beam_search_ex,
    which also takes the CTC operand); without an LM the calls are the ones above."""
    ctc_weight, lm_weight = float(ctc_weight), float(lm_weight)
    if not (0.0 <= lm_weight < float('inf')):
        raise ValueError('lm_weight must be finite and >= 0, got %r' % lm_weight)
    if lm_weight > 0 and lm is None:
        raise ValueError('lm_weight %g needs a language model (lm)' % lm_weight)
    if not 0.0 <= ctc_weight < 1.0:
        raise ValueError('ctc_weight must be in [0, 1), got %r' % ctc_weight)
    if ctc_weight > 0 and ctc_logits is None:
        raise ValueError('ctc_weight %g needs the logits of a CTC head (ctc_logits)' % ctc_weight)
    which, extra = 'beam', ()
    if ctc_logits is not None:
        if ctc_logits.dtype != torch.float32:
            raise _hip.NabuHipError('ctc_logits must be float32, got %s' % ctc_logits.dtype)
        ctc_logits = ctc_logits.contiguous()
        which, extra = 'beam_joint', (_hip.ptr(ctc_logits), ctypes.c_float(ctc_weight))
    if lm is not None and lm_weight > 0:
        if lm.num_labels != cell.output_size:
            raise ValueError('the language model has %d symbols, the decoder %d' % (lm.num_labels, cell.output_size))
        dev = (encoded[0] if isinstance(encoded, (list, tuple)) else encoded).device
        opts = _hip.BeamSearchOpts(size=ctypes.sizeof(_hip.BeamSearchOpts),
                                   ctc_logits=None if ctc_logits is None else _hip.ptr(ctc_logits), ctc_weight=ctc_weight,
                                   lm_table=_hip.ptr(lm.device_table(dev)), lm_order=lm.order, lm_weight=lm_weight)
        which, extra = 'beam_ex', (opts,)
    seq, lengths, scores, aligns, abi = _free_run(which, cell, encoded, encoded_seq_length, beam_width, max_steps,
                                                  length_penalty, temperature, with_alignments, *extra)
    return seq, lengths, scores, (abi.per_memory(aligns) if with_alignments else None)


def sample(cell, encoded, encoded_seq_length, max_steps, seed, offset, with_alignments=False):
    """One sample per utterance from the projected attention cell run free on its own draws (SampleEmbeddingHelper +
    BasicDecoder under dynamic_decode(maximum_iterations=max_steps)): ONE call into the C ABI (nabu_speller_sample:
    the beam search's loop on B rows with nabu_sample_advance in the place of pruning and gathering).  Step t draws
    with the device Philox at (seed, offset + t).  encoded / encoded_seq_length as for beam_search, lists included.
    Returns (sequences [B,time] int32, zero beyond lengths; lengths [B] int32, which count the end label and are
    max_steps for a row that never drew it; nll [B], the summed cross-entropy of the sample; alignments [B,time,Te],
    a list of them for several memories, or None)."""
    seq, lengths, nll, aligns, abi = _free_run('sample', cell, encoded, encoded_seq_length, 1, max_steps, 0.0, 1.0,
                                               with_alignments, int(seed), int(offset))
    return seq[:, 0], lengths[:, 0], nll[:, 0], (abi.per_memory([a[:, 0] for a in aligns]) if with_alignments else None)


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

    supports_ctc_head = True

    def ctc_logits(self, encoded, encoded_seq_length):
        '''the CTC head (ctc_head = True in [decoder]) on the first encoded input: one linear layer to the output's
        classes, whose last one — the end-of-sequence label of the cell — is the CTC blank.  Called inside the
        decoder's scope (the variables are <scope>/ctc_outlayer/{weights,biases}); needs no targets, so a decoder
        can run it next to the cell.  Returns (logits [B,Te,C], their lengths).'''
        if not self.ctc_head:
            raise ValueError('this decoder has no CTC head (ctc_head = True in the [decoder] section)')
        from nabu_amd.neuralnetworks.models.ed_decoders import dnn_decoder
        first = list(encoded.keys())[0]
        return (dnn_decoder.linear(encoded[first], list(self.output_dims.values())[0], 'ctc_outlayer'),
                encoded_seq_length[first])

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
        outputs, lengths = {output_name: logits}, {output_name: logit_seq_length}
        if self.ctc_head:
            # beside the output: losses and decoders index by target name and never see this key
            outputs[output_name + '_ctc'], lengths[output_name + '_ctc'] = self.ctc_logits(encoded, encoded_seq_length)
        return outputs, lengths, ()

    @abstractmethod
    def create_cell(self, encoded, encoded_seq_length, is_training):
        '''create the rnn cell'''

    def zero_state(self, encoded_dim, batch_size):
        '''the decoder zero state: zero cell/hidden states, context and alignments'''
        return ()
