"""Minimum word error rate training of the Speller (Prabhavalkar et al. 2018, "Minimum Word Error Rate Training for
Attention-based Sequence-to-Sequence Models"; the `mwer` objective of ESPnet and Lingvo): the expected number of label
errors over the N-best list of the model's own beam search, plus a small multiple of the reference's cross-entropy.

For utterance b with hypotheses n = 0..N-1 and reference y*:
    nll_n  = sum_{t < len_n} (logsumexp(x[n,t,:]) - x[n,t,y_n[t]])      teacher-forced, end label included
    p_n    = softmax over the valid n of (-nll_n)                        renormalised N-best posterior
    loss_b = sum_n p_n * e_n + lambda * nll_ref                          e_n = edit distance(hyp_n, y* without end label)
and the batch loss is the mean over b.

One step (forward_loss, under the caller's tape): the encoder runs ONCE, in training mode; the beam search
(rnn_decoder.beam_search, one C call) reads its output under no_grad; nabu_mwer_prepare turns the beams into stacked
targets, slot-major (row n * B + b is hypothesis n of utterance b, slot N the reference); ONE nabu_edit_distance call
counts the errors of all N * B hypothesis rows against the reference tiled N times (one call on a tiled reference
rather than a call per slot: the rows are already contiguous, and the tiled reference is one small integer copy);
every encoded input is tiled N + 1 times (nops.tile_rows, a tape node whose gradient sums the replicas in a fixed
order); dynamic_decode scores the (N + 1) * B rows without scheduled sampling; nabu_mwer_loss_grad gives the loss and
the gradient with respect to the logits in one launch.

The only host synchronisation the step adds is the beam search's own read of its step count: the stacked lengths stay on
the device, and dynamic_decode is given the bound max(steps + 1, longest reference) as their host side."""
import numpy as np
import torch

from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, SeqLen
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder

KEYS = ('mwer_nbest', 'mwer_max_steps', 'mwer_ce_weight', 'mwer_start_step')
DEFAULT_CE_WEIGHT = 0.01       # the paper's lambda


def _int_key(conf, key, default, least):
    text = str(conf.get(key, default)).strip()
    try:
        value = int(text)
    except ValueError:
        raise ValueError('%s must be an integer, got %r' % (key, text))
    if value < least:
        raise ValueError('%s must be >= %d, got %r' % (key, least, text))
    return value


def mwer_keys(conf):
    """the `mwer_nbest`, `mwer_max_steps`, `mwer_ce_weight` and `mwer_start_step` keys of the [trainer] section (build
    additions like label_smoothing: absent from the defaults file, off when absent) -> (nbest, max_steps, ce_weight,
    start_step), or None when mwer_nbest is absent or 0.  The other keys without mwer_nbest are an error."""
    nbest = _int_key(conf, 'mwer_nbest', '0', 0)
    if nbest > hip.MWER_MAX_NBEST:
        raise ValueError('mwer_nbest must be in 1..%d (0: off), got %d' % (hip.MWER_MAX_NBEST, nbest))
    if nbest == 0:
        extra = [k for k in KEYS[1:] if k in conf]
        if extra:
            raise ValueError('%s set without mwer_nbest: MWER training is switched on by mwer_nbest = N (1..%d)'
                             % (', '.join(extra), hip.MWER_MAX_NBEST))
        return None
    if 'mwer_max_steps' not in conf:
        raise ValueError('mwer_nbest = %d needs mwer_max_steps, the longest hypothesis the beam search may produce (the '
                         'max_steps of the beam search decoder)' % nbest)
    max_steps = _int_key(conf, 'mwer_max_steps', '0', 1)
    text = str(conf.get('mwer_ce_weight', DEFAULT_CE_WEIGHT)).strip()
    try:
        ce_weight = float(text)
    except ValueError:
        raise ValueError('mwer_ce_weight must be a number, got %r' % text)
    if not (0.0 <= ce_weight < float('inf')):                  # (false for NaN)
        raise ValueError('mwer_ce_weight must be finite and >= 0, got %r' % text)
    return nbest, max_steps, ce_weight, _int_key(conf, 'mwer_start_step', '0', 0)


def check_model(model):
    """MWER needs a recurrent decoder: the search and the scoring pass run its cell"""
    if not isinstance(model.decoder, rnn_decoder.RNNDecoder):
        raise ValueError('mwer_nbest needs a model whose decoder is a recurrent attention decoder (speller); %s is no '
                         'such decoder' % type(model.decoder).__name__)
    if model.decoder.ctc_head:
        raise ValueError('mwer_nbest does not combine with a CTC head yet (ctc_head = True in the [decoder] section)')


def tile_lengths(lens, R, device):
    """a length vector repeated R times, replica-major like nops.tile_rows: the host side on the host, the device side
    on the device"""
    lens = SeqLen.wrap(lens, device)
    return SeqLen(np.tile(lens.host, R), dev_tensor=lens.dev.repeat(R))


def stacked_decode(decoder, encoded, encoded_len, stk_targets, stk_len, bound, R):
    """the scoring pass: every encoded input tiled R times (a tape node each), the training cell, dynamic_decode over the
    stacked targets without scheduled sampling.  Called inside the decoder's scope.  bound: the host-side bound of
    stk_len.  Returns the logits [R * B, bound, C]."""
    names = list(encoded.keys())
    dev = stk_targets.device
    tiled = {e: nops.tile_rows(encoded[e], R) for e in names}
    tiled_len = {e: tile_lengths(encoded_len[e], R, dev) for e in names}
    cell = decoder.create_cell(tiled, tiled_len, True)
    lens = SeqLen(np.full(stk_len.numel(), bound, dtype=np.int32), dev_tensor=stk_len)
    logits, _ = rnn_decoder.dynamic_decode(cell, [tiled[e] for e in names], [tiled_len[e] for e in names], stk_targets,
                                           lens, 0.0, True)
    return logits


def nbest_targets(decoder, encoded, encoded_len, targets, target_len, nbest, max_steps):
    """the search and the glue behind it: (stk_targets, stk_len, hyp_len, valid, errors, bound).  Called inside the
    decoder's scope; nothing here is recorded."""
    names = list(encoded.keys())
    dev = targets.device
    tsl = SeqLen.wrap(target_len, dev)
    B = targets.shape[0]
    with torch.no_grad():
        cell = decoder.create_cell(encoded, encoded_len, False)
        seq, lengths, scores, _ = rnn_decoder.beam_search(
            cell, [encoded[e] for e in names], [encoded_len[e] for e in names], beam_width=nbest, max_steps=max_steps,
            length_penalty=0.0, with_alignments=False)
        bound = max(int(seq.shape[2]) + 1, tsl.max())
        stk_targets, stk_len, hyp_len, valid = hip.mwer_prepare(seq, lengths, scores, targets, tsl.dev,
                                                                cell.output_size, max(bound, targets.shape[1]))
        no_eos = (tsl.dev - 1).clamp_(min=0)
        errors = hip.edit_distance(stk_targets[:nbest * B], hyp_len, targets.repeat(nbest, 1), no_eos.repeat(nbest))
    return stk_targets, stk_len, hyp_len, valid, errors, bound


def forward_loss(model, batch, nbest, max_steps, ce_weight):
    """The MWER forward pass of one device batch under the active tape -> (loss [1], stats); stats: the step's device
    tensors by name (stk_targets, stk_len, errors, valid, risk [B], nll_ref [B]), nothing of which is read here."""
    tname = list(batch['targets'].keys())[0]
    targets = batch['targets'][tname]
    if targets.dtype != torch.int32 or not targets.is_contiguous():
        targets = targets.to(torch.int32).contiguous()
    B = targets.shape[0]
    decoder = model.decoder
    with vs.as_default(model.store):
        # input noise, SpecAugment and encoder dropout apply as in any training step; the search and the scoring pass
        # read the same output
        encoded, encoded_len = model.encoder(inputs=batch['inputs'], input_seq_length=batch['input_seq_length'],
                                             is_training=True)
        with vs.variable_scope(decoder.scope):
            stk_targets, stk_len, _, valid, errors, bound = nbest_targets(
                decoder, encoded, encoded_len, targets, batch['target_seq_length'][tname], nbest, max_steps)
            logits = stacked_decode(decoder, encoded, encoded_len, stk_targets, stk_len, bound, nbest + 1)
    per_utt, risk, nll_ref, dlogits = hip.mwer_loss_grad(logits, stk_targets, stk_len, errors, valid, ce_weight, 1.0 / B)
    loss = hip.sum_(per_utt, 1.0 / B)
    record([logits], [loss], lambda g, d=dlogits: [d])
    return loss, dict(stk_targets=stk_targets, stk_len=stk_len, errors=errors, valid=valid, risk=risk, nll_ref=nll_ref)


def read_stats(stats):
    """(mean expected errors, mean reference nll, share of valid hypotheses) of a step's stats; synchronises"""
    return (float(stats['risk'].mean().item()), float(stats['nll_ref'].mean().item()),
            float(stats['valid'].float().mean().item()))
