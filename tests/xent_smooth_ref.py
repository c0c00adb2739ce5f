"""Float64 restatement of the label-smoothed cross-entropy losses (nabu_xent_smooth_loss_grad and its wide twin,
loss_functions.average_cross_entropy / sum_cross_entropy with label_smoothing), written from the formula: with C
classes the target of a frame with label y is q = (1 - e) * onehot(y) + e / C, and per frame t inside the mask

    loss_t = lz - (1 - e) * x_y - e * mean_c(x_c),   lz = logsumexp(x)
    d_c    = s * (softmax_c - (1 - e) * [c = y] - e / C)

The two masks: `average` counts t < logit_len[b] and divides by target_len[b]; `sum` counts t < target_len[b] and
divides by one."""
import numpy as np


def per_utterance(logits, targets, mask_len, divisor, smoothing, grad_scale=1.0):
    """(loss [B], dlogits [B,L,C]) in float64: loss[b] = sum_{t < mask_len[b]} loss_t / divisor[b], dlogits =
    grad_scale * d loss[b] / d logits (zero rows past the mask).  logits [B,L,C]; targets [B, >= L]."""
    x = np.asarray(logits, np.float64)
    B, L, C = x.shape
    e = float(smoothing)
    y = np.asarray(targets)[:, :L].astype(np.int64)
    n = np.clip(np.asarray(mask_len, np.int64), 0, L)
    div = np.asarray(divisor, np.float64)
    m = x.max(-1, keepdims=True)
    lz = m[..., 0] + np.log(np.exp(x - m).sum(-1))
    x_y = np.take_along_axis(x, y[:, :, None], 2)[:, :, 0]
    # (the same number as lz - (1 - e) * x_y - e * mean(x), summed as two non-negative parts)
    frame = (1.0 - e) * (lz - x_y) + e * (lz - x.mean(-1))
    live = np.arange(L)[None, :] < n[:, None]
    loss = np.where(live, frame, 0.0).sum(1) / div
    hot = np.zeros((B, L, C))
    np.put_along_axis(hot, y[:, :, None], 1.0 - e, 2)
    d = ((np.exp(x - lz[..., None]) - e / C) - hot) * live[:, :, None] * (grad_scale / div)[:, None, None]
    return loss, d


def average(logits, targets, logit_len, target_len, smoothing, grad_scale=1.0):
    """average_cross_entropy's mask and divisor: t < logit_len[b], / target_len[b]"""
    return per_utterance(logits, targets, logit_len, target_len, smoothing, grad_scale)


def summed(logits, targets, target_len, smoothing, grad_scale=1.0):
    """sum_cross_entropy's mask and divisor: t < target_len[b], / 1"""
    return per_utterance(logits, targets, target_len, np.ones(len(target_len)), smoothing, grad_scale)


def entropy(C, smoothing):
    """H(q) of the smoothed target over C classes: the least a frame's loss can be"""
    e = float(smoothing)
    hot, cold = 1.0 - e + e / C, e / C
    h = -hot * np.log(hot)
    if cold > 0 and C > 1:
        h -= (C - 1) * cold * np.log(cold)
    return h
