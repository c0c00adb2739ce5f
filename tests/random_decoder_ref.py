"""Host restatement of the sampled decode's step (nabu_sample_advance, decode.hip) GIVEN the drawn ids: the
bookkeeping of tf.contrib.seq2seq.SampleEmbeddingHelper + BasicDecoder under dynamic_decode as the reference's
RandomDecoder uses them (decoders/random_decoder.py:80-120; TF-1.8 recalled), and the float64 cross-entropy of a
sample.  The draw itself is oracle/philox.py's reference_draw."""
import numpy as np


def lse(logits):
    """float64 log-sum-exp over the last axis"""
    x = np.asarray(logits, np.float64)
    m = x.max(-1)
    return m + np.log(np.exp(x - m[..., None]).sum(-1))


def xent(logits, ids):
    """float64 [B]: logsumexp(logits[b]) - logits[b, ids[b]]"""
    x = np.asarray(logits, np.float64)
    return lse(x) - x[np.arange(x.shape[0]), ids]


class State(object):
    """sequences [B, max_steps], lengths, finished [B] int32, nll [B] float64 of a sampled decode"""

    def __init__(self, B, max_steps):
        self.max_steps = max_steps
        self.sequences = np.zeros((B, max_steps), np.int32)
        self.lengths, self.finished = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.nll = np.zeros(B, np.float64)

    def advance(self, t, logits, ids):
        """step t with the drawn ids [B]; returns all_finished (0 or 1)"""
        C = logits.shape[1]
        live = self.finished == 0
        self.sequences[:, t] = np.where(live, ids, 0)
        self.nll += np.where(live, xent(logits, ids), 0.0)
        ends = live & ((ids == C - 1) | (t + 1 >= self.max_steps))
        self.lengths[ends] = t + 1
        self.finished[ends] = 1
        return int(self.finished.all())


def sample_nll(logits, sequences, lengths):
    """float64 [B]: the summed cross-entropy of sequences[b, :lengths[b]] under logits [B, L, C]"""
    out = np.zeros(len(lengths), np.float64)
    for t in range(logits.shape[1]):
        rows = t < lengths
        out[rows] += xent(logits[rows, t], sequences[rows, t])
    return out
