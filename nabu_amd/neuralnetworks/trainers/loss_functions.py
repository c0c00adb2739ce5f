"""Training losses (reference: nabu/neuralnetworks/trainers/loss_functions.py).

Each loss is one fused HIP kernel that produces the per-utterance loss AND the
gradient w.r.t. the logits in the same pass (as tf.nn.ctc_loss does); the
gradient is handed to the tape."""
import functools

import torch

from nabu_amd import ops as hip
from nabu_amd.autodiff import record, SeqLen, UNIT
from nabu_amd.neuralnetworks.components import ops

# device status words of the CTC and transducer kernels launched since the last check
pending_status = []

# class counts from which the cross-entropy losses run nabu_xent_wide_loss_grad (one wave per frame) instead of
# nabu_xent_loss_grad (one thread per frame, written for a few dozen classes): the 3100 HMM states of DNN/WSJ
WIDE_XENT_MIN_CLASSES = 1024


def _xent(logits, targets, logit_len_dev, target_len_dev, grad_scale, label_smoothing=0.0):
    '''the cross-entropy kernel for the class count of `logits`; without smoothing the entry points (and so the
    launches and their arguments) are the ones a configuration without the label_smoothing key always had'''
    wide = logits.shape[-1] >= WIDE_XENT_MIN_CLASSES
    if label_smoothing == 0:
        fn = hip.xent_wide_loss_grad if wide else hip.xent_loss_grad
        return fn(logits, targets, logit_len_dev, target_len_dev, grad_scale)
    fn = hip.xent_wide_smooth_loss_grad if wide else hip.xent_smooth_loss_grad
    return fn(logits, targets, logit_len_dev, target_len_dev, grad_scale, label_smoothing)


def label_smoothing_key(conf):
    """the `label_smoothing` key of the [trainer] section (a build addition like layer_norm and the SpecAugment keys:
    absent from the defaults file, 0 when absent): the probability mass spread uniformly over the classes of every
    output, 0 <= value < 1"""
    text = str(conf.get('label_smoothing', '0')).strip()
    try:
        value = float(text)
    except ValueError:
        raise ValueError('label_smoothing must be a number, got %r' % text)
    if not 0.0 <= value < 1.0:                     # (false for nan)
        raise ValueError('label_smoothing must be in [0, 1), got %r' % text)
    return value


def ctc_weight_key(conf):
    """the `ctc_weight` key of the [trainer] section (a build addition like label_smoothing: absent from the defaults
    file, 0 when absent): the weight w of the auxiliary CTC loss on the model's CTC head (ctc_head = True in the model's
    [decoder] section), loss = (1 - w) * attention loss + w * CTC loss, 0 <= w < 1"""
    text = str(conf.get('ctc_weight', '0')).strip()
    try:
        value = float(text)
    except ValueError:
        raise ValueError('ctc_weight must be a number, got %r' % text)
    if not 0.0 <= value < 1.0:                     # (false for nan)
        raise ValueError('ctc_weight must be in [0, 1), got %r' % text)
    return value


def factory(loss_function, label_smoothing=0.0, ctc_weight=0.0):
    '''get a callable loss(targets, logits, logit_seq_length, target_seq_length)
    (reference loss_functions.py:7-28).  label_smoothing (not the reference's: the [trainer] key of that name) is
    bound into the cross-entropy losses: every output is scored against (1 - e) * onehot + e / C over its own C
    classes.  The LossEvaluator asks for its loss without it, so validation losses are the unsmoothed quantity
    whatever the training run smooths with.  ctc_weight (the [trainer] key of that name) is bound into them the same
    way: (1 - w) * the loss + w * the CTC loss of the model's CTC head; the LossEvaluator asks without it as well, so
    validation is the attention loss, comparable across weights.'''
    label_smoothing, ctc_weight = float(label_smoothing), float(ctc_weight)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError('label_smoothing must be in [0, 1), got %r' % label_smoothing)
    if not 0.0 <= ctc_weight < 1.0:
        raise ValueError('ctc_weight must be in [0, 1), got %r' % ctc_weight)
    # (without the keys: the function itself, as ever)
    extra = dict(label_smoothing=label_smoothing) if label_smoothing else {}
    if ctc_weight:
        extra['ctc_weight'] = ctc_weight
    if loss_function == 'average_cross_entropy':
        return functools.partial(average_cross_entropy, **extra) if extra else average_cross_entropy
    elif loss_function == 'CTC':
        if label_smoothing:
            raise ValueError('label_smoothing is defined for the cross-entropy losses only (average_cross_entropy, '
                             'sum_cross_entropy), not for CTC')
        if ctc_weight:
            raise ValueError('ctc_weight adds a CTC term to the cross-entropy losses (average_cross_entropy, '
                             'sum_cross_entropy); loss = CTC is that term alone')
        return CTC
    elif loss_function == 'sum_cross_entropy':
        return functools.partial(sum_cross_entropy, **extra) if extra else sum_cross_entropy
    elif loss_function == 'transducer':
        if label_smoothing:
            raise ValueError('label_smoothing is defined for the cross-entropy losses only (average_cross_entropy, '
                             'sum_cross_entropy), not for the transducer loss')
        if ctc_weight:
            raise ValueError('ctc_weight adds a CTC term to the cross-entropy losses (average_cross_entropy, '
                             'sum_cross_entropy); a transducer model has no CTC head')
        return transducer
    elif loss_function in ('average_sigmoid_cross_entropy', 'marigin'):
        raise Exception('loss function %s is outside the MI355X hot path' % loss_function)
    else:
        raise Exception('unknown loss function %s' % loss_function)


def _labels(t):
    if t.dtype != torch.int32 or not t.is_contiguous():
        t = t.to(torch.int32).contiguous()
    return t


def _single_logits(name, logits, t):
    '''the losses over ONE logit tensor per output refuse the outputs of a transducer model'''
    if t + '_pred' in logits:
        raise ValueError('loss = %s on the outputs of a transducer model (decoder = transducer): its transcription logits '
                         'alone are no model of the labels; use loss = transducer' % name)


def _total(losses):
    '''sum over the outputs (reference loss_functions.py:212: tf.reduce_sum over the per-output
    losses).  With several outputs the sum is a node of its own and is recorded on the tape, so that
    the backward pass reaches every term (each gets the unit gradient).'''
    if len(losses) == 1:
        return losses[0]
    total = losses[0].clone()
    for l in losses[1:]:
        hip.axpy_(total, l)
    record(losses, [total], lambda g: [UNIT] * len(losses))
    return total


def _ctc_term(t, targets, logits, logit_seq_length, target_seq_length, ctc_weight):
    '''w * mean_b(-log p_ctc(targets[b, :target_len[b] - 1] | the CTC head's logits)): the targets without their end
    label, which is the head's blank.  The status word goes on pending_status, so an utterance whose targets do not fit
    into its encoded length raises like any CTC loss.'''
    key = t + '_ctc'
    if key not in logits:
        raise ValueError('ctc_weight needs a model with a CTC head (ctc_head = True in the [decoder] section): no '
                         'output %r' % key)
    lg = logits[key]
    B = lg.shape[0]
    lsl, tsl = SeqLen.wrap(logit_seq_length[key], lg.device), SeqLen.wrap(target_seq_length[t], lg.device)
    no_eos = (tsl.dev - 1).clamp_(min=0)
    nll, dlogits, status = hip.ctc_loss_grad(lg.contiguous(), lsl.dev, _labels(targets[t]), no_eos, ctc_weight / B)
    pending_status.append(status)
    loss = hip.sum_(nll, ctc_weight / B)
    record([lg], [loss], lambda g, d=dlogits: [d])
    return loss


def CTC(targets, logits, logit_seq_length, target_seq_length):
    '''CTC loss (reference loss_functions.py:180-214): mean over the batch of
    -log p(targets | logits), summed over the outputs; blank = last class.'''
    losses = []
    for t in targets:
        _single_logits('CTC', logits, t)
        lg = logits[t]
        B = lg.shape[0]
        lsl, tsl = SeqLen.wrap(logit_seq_length[t], lg.device), SeqLen.wrap(target_seq_length[t], lg.device)
        labels, _ = ops.dense_sequence_to_sparse(_labels(targets[t]), tsl)
        nll, dlogits, status = hip.ctc_loss_grad(lg.contiguous(), lsl.dev, labels, tsl.dev, 1.0 / B)
        pending_status.append(status)
        loss = hip.sum_(nll, 1.0 / B)
        record([lg], [loss], lambda g, d=dlogits: [d])
        losses.append(loss)
    return _total(losses)


def transducer(targets, logits, logit_seq_length, target_seq_length):
    '''RNN transducer loss with the additive joint (not in the reference; nabu_transducer_loss_grad): mean over the
    batch of -log p(targets | f, g), summed over the outputs, with f = logits[o] the transcription logits and
    g = logits[o + '_pred'] the prediction logits of a `decoder = transducer` model; blank = last class.  One tape node
    with two inputs.  The status word goes on pending_status: an utterance with a label outside the classes or a
    length outside its tensor raises at the next check.'''
    losses = []
    for t in targets:
        key = t + '_pred'
        if key not in logits:
            raise ValueError('loss = transducer needs the prediction logits of a transducer model (decoder = transducer '
                             'in the [decoder] section): no output %r' % key)
        f, g = logits[t], logits[key]
        B = f.shape[0]
        lsl, tsl = SeqLen.wrap(logit_seq_length[t], f.device), SeqLen.wrap(target_seq_length[t], f.device)
        labels = _labels(torch.as_tensor(targets[t]).to(f.device))
        nll, df, dg, status = hip.transducer_loss_grad(f.contiguous(), g.contiguous(), lsl.dev,
                                                       labels if labels.numel() else None, tsl.dev, 1.0 / B)
        status.error = transducer_status_error
        pending_status.append(status)
        loss = hip.sum_(nll, 1.0 / B)
        record([f, g], [loss], lambda gr, a=df, b=dg: [a, b])
        losses.append(loss)
    return _total(losses)


def check_model(loss_function, decoder):
    '''loss and decoder belong together: loss = transducer reads the two outputs of `decoder = transducer`, and the other
    losses read a single logit tensor, which that decoder does not give.  Raises ValueError at construction.'''
    from nabu_amd.neuralnetworks.models.ed_decoders import transducer as transducer_model
    is_transducer = isinstance(decoder, transducer_model.Transducer)
    if loss_function == 'transducer' and not is_transducer:
        raise ValueError('loss = transducer needs a transducer model (decoder = transducer in the [decoder] section), '
                         'got %s' % type(decoder).__name__)
    if is_transducer and loss_function != 'transducer':
        raise ValueError('a transducer model (decoder = transducer) is trained with loss = transducer, not loss = %s: '
                         'its transcription logits alone are no model of the labels' % loss_function)


def average_cross_entropy(targets, logits, logit_seq_length, target_seq_length, label_smoothing=0.0, ctc_weight=0.0):
    '''cross entropy averaged over timesteps (reference loss_functions.py:155-165):
    mean_b( sum_{t<logit_len} xent / target_len ), summed over the outputs.  label_smoothing, ctc_weight: see
    factory.'''
    losses = []
    for t in targets:
        _single_logits('average_cross_entropy', logits, t)
        lg = logits[t]
        B = lg.shape[0]
        lsl, tsl = SeqLen.wrap(logit_seq_length[t], lg.device), SeqLen.wrap(target_seq_length[t], lg.device)
        scale = (1.0 - ctc_weight) / B if ctc_weight else 1.0 / B
        per_utt, dlogits = _xent(lg.contiguous(), _labels(targets[t]), lsl.dev, tsl.dev, scale, label_smoothing)
        loss = hip.sum_(per_utt, scale)
        record([lg], [loss], lambda g, d=dlogits: [d])
        losses.append(loss)
        if ctc_weight:
            losses.append(_ctc_term(t, targets, logits, logit_seq_length, target_seq_length, ctc_weight))
    return _total(losses)


def sum_cross_entropy(targets, logits, logit_seq_length, target_seq_length, label_smoothing=0.0, ctc_weight=0.0):
    '''cross entropy summed over timesteps (reference loss_functions.py:142-153): the mask is the
    TARGET length here and nothing is divided: mean_b( sum_{t<target_len} xent ), summed over the
    outputs.  Same kernel as average_cross_entropy with a divisor of one.  label_smoothing, ctc_weight: see
    factory.'''
    losses = []
    for t in targets:
        _single_logits('sum_cross_entropy', logits, t)
        lg = logits[t]
        B = lg.shape[0]
        tsl = SeqLen.wrap(target_seq_length[t], lg.device)
        ones = torch.ones_like(tsl.dev)
        scale = (1.0 - ctc_weight) / B if ctc_weight else 1.0 / B
        per_utt, dlogits = _xent(lg.contiguous(), _labels(targets[t]), tsl.dev, ones, scale, label_smoothing)
        loss = hip.sum_(per_utt, scale)
        record([lg], [loss], lambda g, d=dlogits: [d])
        losses.append(loss)
        if ctc_weight:
            losses.append(_ctc_term(t, targets, logits, logit_seq_length, target_seq_length, ctc_weight))
    return _total(losses)


def ctc_status_error(code):
    '''the exception a non-zero status word of the CTC kernel stands for'''
    return Exception('CTC: Not enough time for target transition sequence '
                     '(utterance %d of the batch)' % (code - 1))


def transducer_status_error(code):
    '''the exception a non-zero status word of the transducer kernel stands for'''
    return Exception('transducer: invalid utterance %d of the batch' % (code - 1))


def status_error(status, code):
    '''the exception for a non-zero `code` read from the status word `status`: the kernel that owns the word says what
    it means (an `error` attribute on the tensor); a word without one is a CTC kernel's'''
    return getattr(status, 'error', ctc_status_error)(code)


def take_pending_status():
    '''the status words of the CTC kernels launched since the last check; the caller reads them (the overlapped
    training loop does, one step late: trainers/readback.py)'''
    global pending_status
    todo, pending_status = pending_status, []
    return todo


def check_status():
    '''raise (as tf.nn.ctc_loss does) if any CTC utterance had no valid alignment'''
    for s in take_pending_status():
        code = int(s.item())
        if code:
            raise status_error(s, code)
    # a persistent recurrent kernel that gave up (bounded-spin timeout) leaves the results of the
    # step invalid and its status word set: raise here, where the training / validation loops
    # already synchronise
    hip.check_persist_status()
