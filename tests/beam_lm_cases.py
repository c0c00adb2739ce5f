"""Cases of the pruning step and the attention beam search with a label n-gram (nabu_beam_prune_lm,
nabu_speller[_multi]_beam_search_ex) and their float64 references: tests/beam_joint_cases.py extended by the LM term
(plain NumPy; importable without a GPU).  As there, every case is built from a seed that a CPU search
(decode_cases.find_seeds) accepted with a float64 margin above MARGIN; tests/test_beam_lm_cases.py asserts that again
for every committed seed."""
import numpy as np

from tests import beam_joint_cases as J
from tests import ngram_lm_ref as NR

MARGIN, LAM, FMAX = J.MARGIN, J.LAM, J.FMAX
GAMMA = 0.5


# ---------------------------------------------------------------------------------------------------------------
# one pruning step: the geometries of beam_joint_cases x (delta or not) x order x beam mix
MIXES = ('finished', 'live', 'both')
PRUNE_KEYS = [(geo, with_delta, order, mix) for geo in sorted(J.PRUNE_CASES) for with_delta in (True, False)
              for order in (1, 3) for mix in MIXES]


def prune_id(key):
    (W, C, _, _), with_delta, order, mix = key
    return 'W%d-C%d-%s-n%d-%s' % (W, C, 'ctc' if with_delta else 'att', order, mix)


def prune_inputs(key, seed):
    """logits, delta (or None), table float32, ctx int32 [B,W], logprobs, lengths, finished, seen.  The contexts are
    those of hypotheses longer than n-1 labels (any row of the table), so next() wraps."""
    (W, C, _, _), with_delta, order, mix = key
    logits, delta, logprobs, lengths, finished, _ = J.prune_inputs(J.PRUNE_B, W, C, seed)
    if mix == 'finished':
        finished[:] = 1
    elif mix == 'live':
        finished[:] = 0
    else:
        finished[:, 0], finished[:, 1] = 1, 0
    delta[finished > 0] = 0
    rng = np.random.default_rng([seed, W, C, order, 5])
    ctx = rng.integers(0, C ** (order - 1), (J.PRUNE_B, W)).astype(np.int32)
    lengths = (lengths + order).astype(np.int32)
    return (logits, delta if with_delta else None, NR.random_table(C, order, seed), ctx, logprobs, lengths, finished,
            finished.copy())


def prune_lm_reference(logits, delta, lam, table, order, gamma, ctx, logprobs, lengths, finished, temp, lpw):
    """nabu_beam_prune_lm in float64 (beam_joint_cases.prune_joint_reference with the LM term): all_lp, all_ids,
    all_len [B, W*C + W], order [B,W], gap [B], ctx_out [B,W]"""
    B, W, C = logits.shape
    x = logits.astype(np.float64) / temp
    nlp = x - x.max(-1, keepdims=True)
    nlp = nlp - np.log(np.exp(nlp).sum(-1, keepdims=True))
    if delta is not None:
        nlp = (1.0 - lam) * nlp + lam * delta.astype(np.float64)
    nlp = nlp + gamma * table.astype(np.float64)[ctx]
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
    sel = full[:, :W]
    st = sel >= W * C
    parent = np.where(st, sel - W * C, sel // C)
    bi = np.arange(B)[:, None]
    pctx = ctx[bi, parent].astype(np.int64)
    nctx = C ** (order - 1)
    ctx_out = np.where(st, pctx, (pctx * C + all_ids[bi, sel]) % nctx).astype(np.int32)
    return dict(all_lp=all_lp, all_ids=all_ids, all_len=all_len, order=sel, gap=(top[:, :-1] - top[:, 1:]).min(1),
                ctx_out=ctx_out)


def prune_reference(key, seed, gamma=GAMMA, lam=LAM):
    (W, C, lpw, temp), with_delta, order, mix = key
    logits, delta, table, ctx, logprobs, lengths, finished, _ = prune_inputs(key, seed)
    return prune_lm_reference(logits, delta, lam, table, order, gamma, ctx, logprobs, lengths, finished, temp, lpw)


def prune_ok(key, seed):
    """a float64 margin, and (where a beam is live) a selection the LM term changes"""
    ref = prune_reference(key, seed)
    if not ref['gap'].min() > MARGIN:
        return False
    return key[3] == 'finished' or not np.array_equal(ref['order'], prune_reference(key, seed, gamma=0.0)['order'])


# prune_id(key) -> seed: find_seeds(lambda s: prune_ok(key, s))
PRUNE_SEEDS = dict({prune_id(k): 0 for k in PRUNE_KEYS}, **{
    'W8-C5-ctc-n1-live': 1, 'W16-C40-ctc-n1-finished': 1, 'W16-C40-ctc-n1-live': 1, 'W16-C40-ctc-n3-finished': 1,
    'W16-C40-ctc-n3-live': 4, 'W16-C40-ctc-n3-both': 2, 'W16-C40-att-n1-finished': 1, 'W16-C40-att-n1-live': 1,
    'W16-C40-att-n3-finished': 1, 'W16-C40-att-n3-live': 2, 'W16-C40-att-n3-both': 1})


# ---------------------------------------------------------------------------------------------------------------
# the whole search: the SEARCH geometry of beam_joint_cases (exhaustive at W = 40), a bigram over its C = 4 symbols
SEARCH_ORDER = 2
SEARCH_KINDS = ('vanilla', 'two_inputs')
SEARCH_LAMS = (0.0, LAM)


def search_table(seed):
    return NR.random_table(J.SEARCH['C'], SEARCH_ORDER, seed)


_tables = {}


def lm_table(kind, seed, max_len=2):
    """per utterance {labels: (log p_att(labels . eos), log p_ctc(labels), log p_lm(labels . eos))}: the brute-force
    table of beam_joint_cases with the LM term (computed once per kind and seed)"""
    if (kind, seed) not in _tables:
        logp = search_table(seed).astype(np.float64)
        C = J.SEARCH['C']
        _tables[kind, seed] = [{g: (a, c, NR.sequence_logprob(logp, g, C, SEARCH_ORDER)) for g, (a, c) in t.items()}
                               for t in J.joint_table(kind, seed, max_len)]
    return _tables[kind, seed]


def fused_score(att, ctc, lm, lam, gamma=GAMMA):
    return J.joint_score(att, ctc, lam) + gamma * lm


def search_margin(kind, seed, lam):
    """the smallest float64 gap over the batch between the best and the second best fused score"""
    gaps = []
    for table in lm_table(kind, seed):
        s = sorted((fused_score(a, c, l, lam) for a, c, l in table.values()), reverse=True)
        gaps.append(s[0] - s[1])
    return min(gaps)


def search_ok(kind, seed):
    return all(search_margin(kind, seed, lam) > MARGIN for lam in SEARCH_LAMS)


# kind -> seed: find_seeds(lambda s: search_ok(kind, s))
SEARCH_SEEDS = {'vanilla': 0, 'two_inputs': 0}
