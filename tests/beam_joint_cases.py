"""Cases of the joint CTC/attention pruning step and beam search, and their float64 references (plain NumPy;
importable without a GPU).  The device works in float32, so a case can be held to the float64 SELECTION only where
float64 leaves a margin float32 cannot close: every case here is built from a seed that a CPU search (find_seeds of
tests/decode_cases.py) accepted with a margin above MARGIN, and tests/test_beam_joint_cases.py asserts that again for
every committed seed."""
import itertools

import numpy as np

from oracle import decode_oracle as D
from oracle import nabu_oracle as O
from tests import multi_speller_ref as MR

MARGIN = 1e-3
LAM = 0.3
FMAX = float(np.finfo(np.float32).max)


# ---------------------------------------------------------------------------------------------------------------
# one pruning step
def prune_inputs(B, W, C, seed):
    """logits, delta [B,W,C]; logprobs, lengths, finished, seen [B,W].  A finished beam's delta row is zero, as the
    score kernel leaves it; some deltas are log 0 (-1e30)."""
    rng = np.random.default_rng([seed, B, W, C])
    logits = rng.normal(0, 2, (B, W, C)).astype(np.float32)
    delta = (-rng.exponential(3.0, (B, W, C))).astype(np.float32)
    delta[rng.uniform(size=(B, W, C)) < 0.1] = -1e30
    logprobs = (-rng.uniform(0, 5, (B, W))).astype(np.float32)
    lengths = rng.integers(0, 7, (B, W)).astype(np.int32)
    finished = (rng.uniform(size=(B, W)) < 0.3).astype(np.int32)
    delta[finished > 0] = 0
    return logits, delta, logprobs, lengths, finished, finished.copy()


def prune_joint_reference(logits, delta, lam, logprobs, lengths, finished, temp, lpw):
    """nabu_beam_prune_joint in float64 (tests/test_hip_decode.py: prune_reference, with the CTC term): all_lp,
    all_ids, all_len [B, W*C + W], order [B, W], and gap [B]: the smallest difference between neighbouring scores
    among the W + 1 best candidates"""
    B, W, C = logits.shape
    x = logits.astype(np.float64) / temp
    nlp = x - x.max(-1, keepdims=True)
    nlp = nlp - np.log(np.exp(nlp).sum(-1, keepdims=True))
    nlp = (1.0 - lam) * nlp + lam * delta.astype(np.float64)
    nlp = np.where(finished[:, :, None] > 0, -FMAX, nlp)
    cand_lp = (logprobs.astype(np.float64)[:, :, None] + nlp).reshape(B, W * C)
    cand_ids = np.tile(np.arange(C), (B, W))
    cand_len = np.repeat(lengths, C, 1) + (cand_ids != C - 1)
    all_lp = np.concatenate([cand_lp, np.where(finished > 0, logprobs.astype(np.float64), -FMAX)], 1)
    all_ids = np.concatenate([cand_ids, np.full((B, W), C - 1)], 1)
    all_len = np.concatenate([cand_len, lengths], 1)
    pen = 1.0 if lpw == 0 else ((5.0 + all_len) ** lpw) / (6.0 ** lpw)
    scores = all_lp / pen
    full = np.argsort(-scores, 1, kind='stable')
    top = np.take_along_axis(scores, full[:, :W + 1], 1)
    return dict(all_lp=all_lp, all_ids=all_ids, all_len=all_len, order=full[:, :W], gap=(top[:, :-1] - top[:, 1:]).min(1))


# (W, C, length penalty, temperature) -> seed: find_seeds(lambda s: prune_gap(W, C, lpw, temp, s) > MARGIN)
PRUNE_B = 3
PRUNE_CASES = {(4, 6, 0.0, 1.0): 0, (16, 40, 1.0, 1.0): 3, (8, 5, 0.7, 2.0): 0, (5, 3, 0.0, 1.0): 0}


def prune_gap(W, C, lpw, temp, seed):
    logits, delta, logprobs, lengths, finished, _ = prune_inputs(PRUNE_B, W, C, seed)
    return float(prune_joint_reference(logits, delta, LAM, logprobs, lengths, finished, temp, lpw)['gap'].min())


# ---------------------------------------------------------------------------------------------------------------
# the whole search on a tiny Speller: C = 4, three steps, a beam wide enough to keep every hypothesis
SEARCH = dict(B=3, U=32, E=32, Te=7, C=4, S=3, W=40, enc_len=np.array([7, 4, 5], np.int32))
SEARCH_KINDS = {'vanilla': ('vanilla', 1), 'location_aware': ('location_aware', 1), 'two_inputs': ('vanilla', 2)}
AUX = dict(Te=5, E=16, enc_len=np.array([3, 5, 4], np.int32))       # the second encoded input of 'two_inputs'
K_LOC, F_LOC = 3, 2


def search_case(kind, seed):
    """(attention, float64 parameters in the form of tests/multi_speller_ref.py, [encoded float32], [lengths], the CTC
    head's logits float32 [B,Te,C] on the first encoded input)"""
    attention, M = SEARCH_KINDS[kind]
    c = SEARCH
    rng = np.random.default_rng([seed, M, len(attention)])
    shapes = [(c['Te'], c['E'], c['enc_len'])] + [(AUX['Te'], AUX['E'], AUX['enc_len'])] * (M - 1)
    p = MR.make_params(rng, c['C'], c['U'], [s[1] for s in shapes], 1, attention, K_LOC, F_LOC)
    p = _float32_values(p)
    encs = []
    for Te, E, el in shapes:
        e = rng.normal(size=(c['B'], Te, E)).astype(np.float32)
        encs.append(e * (np.arange(Te)[None, :, None] < el[:, None, None]))
    ctc_logits = rng.normal(0, 1.5, (c['B'], c['Te'], c['C'])).astype(np.float32)
    return attention, p, encs, [s[2] for s in shapes], ctc_logits


def _float32_values(p):
    """the float64 parameters rounded to what the device holds"""
    if isinstance(p, dict):
        return {k: _float32_values(v) for k, v in p.items()}
    if isinstance(p, list):
        return [_float32_values(v) for v in p]
    return p.astype(np.float32).astype(np.float64)


def sequences(C, max_len):
    return [g for n in range(max_len + 1) for g in itertools.product(range(C - 1), repeat=n)]


def joint_table(kind, seed, max_len=2):
    """per utterance {labels: (log p_att(labels . eos), log p_ctc(labels))} in float64 for every label sequence of at
    most max_len labels: the attention term teacher-forced (oracle.speller_fwd; several inputs: its M-memory
    restatement tests/multi_speller_ref.py), the CTC term by oracle.ctc_loss on the head's logits"""
    attention, p, encs, enc_lens, ctc_logits = search_case(kind, seed)
    C, B = SEARCH['C'], SEARCH['B']
    seqs = sequences(C, max_len)
    out = []
    for b in range(B):
        e1 = [e[b:b + 1].astype(np.float64) for e in encs]
        l1 = [l[b:b + 1] for l in enc_lens]
        table = {}
        for g in seqs:
            tg = np.array([list(g) + [C - 1]])
            if len(encs) == 1:
                single = dict(p['mem'][0], lstm=p['lstm'], out_kernel=p['out_kernel'], out_bias=p['out_bias'])
                lg = O.speller_fwd(e1[0], l1[0], tg, [len(g) + 1], single, attention)[0]
            else:
                lg = MR.multi_speller_fwd(e1, l1, tg, [len(g) + 1], p, attention)[0]
            att = float(sum(D._log_softmax(lg[0, t])[k] for t, k in enumerate(tg[0])))
            lab = np.array([list(g) + [0] * (max_len - len(g))], np.int32).reshape(1, max_len)
            nll, _ = O.ctc_loss(ctc_logits[b:b + 1].astype(np.float64), l1[0], lab, np.array([len(g)], np.int32))
            table[g] = (att, -float(nll[0]))
        out.append(table)
    return out


def joint_score(att, ctc, lam=LAM):
    return (1.0 - lam) * att + lam * max(ctc, -1e30)


def search_margin(kind, seed):
    """the smallest float64 gap over the batch between the best and the second best joint score"""
    gaps = []
    for table in joint_table(kind, seed):
        s = sorted((joint_score(a, c) for a, c in table.values()), reverse=True)
        gaps.append(s[0] - s[1])
    return min(gaps)


# kind -> seed: find_seeds(lambda s: search_margin(kind, s) > MARGIN)
SEARCH_SEEDS = {'vanilla': 0, 'location_aware': 0, 'two_inputs': 0}
