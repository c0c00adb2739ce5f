"""Cases of the MWER end-to-end tests on the tiny Speller of tests/beam_joint_cases.py (B = 3, U = E = 32, C = 4, three
steps; kinds vanilla, location_aware, two_inputs) with N = 4 hypotheses, and their float64 chain: brute-force N-best,
tile, multi_speller_fwd, the reference loss, multi_speller_bwd, the sum over the slots.  Plain NumPy, importable without
a GPU.  The device's N-best can be held to the float64 one only where float64 leaves a margin: every committed seed has
neighbouring candidate scores at least beam_joint_cases.MARGIN apart around the kept ones at every step
(tests/test_mwer_cases.py asserts it on the CPU)."""
import numpy as np

from tests import beam_joint_cases as J
from tests import multi_speller_ref as MR
from tests import mwer_ref

N = 4
CE_WEIGHT = 0.25
KINDS = sorted(J.SEARCH_KINDS)
# kind -> seed: the first seed s >= 0 with nbest_margin(kind, s) >= J.MARGIN
SEEDS = {'location_aware': 0, 'two_inputs': 0, 'vanilla': 0}


def case(kind, seed=None):
    """(attention, float64 parameters, [encoded float32], [lengths], targets [B,4] int32, target_len [B])"""
    seed = SEEDS[kind] if seed is None else seed
    attention, p, encs, enc_lens, _ = J.search_case(kind, seed)
    c = J.SEARCH
    rng = np.random.default_rng([seed, 77])
    target_len = np.array([3, 1, 4], np.int32)                # the end label counts; one empty reference
    targets = rng.integers(0, c['C'] - 1, (c['B'], 4)).astype(np.int32)
    for b, tl in enumerate(target_len):
        targets[b, tl - 1] = c['C'] - 1
        targets[b, tl:] = 0
    return attention, p, encs, enc_lens, targets, target_len


def brute_force(kind, seed=None):
    """the float64 N-best: (per utterance [(labels without end labels, length, logprob)] best first, margin, steps)"""
    attention, p, encs, enc_lens, _, _ = case(kind, seed)
    beams, gap, T = MR.brute_force_beam_search([e.astype(np.float64) for e in encs], enc_lens, p, N, J.SEARCH['S'],
                                               attention)
    end = J.SEARCH['C'] - 1
    out = [[(tuple(k for k in lab if k != end), ln, lp) for lab, ln, lp, _fin, _, _al in utt] for utt in beams]
    return out, gap, T


def nbest_margin(kind, seed):
    return brute_force(kind, seed)[1]


def float64_chain(kind, stk_targets, stk_len, errors, valid, seed=None):
    """the scoring pass and its gradient in float64 on given stacked targets: (loss scalar, [d encoded_m], parameter
    gradients in the form of the parameters)"""
    attention, p, encs, enc_lens, _, _ = case(kind, seed)
    B = encs[0].shape[0]
    R = N + 1
    tiled = [mwer_ref.tile(e.astype(np.float64), R) for e in encs]
    tiled_lens = [np.tile(np.asarray(l), R) for l in enc_lens]
    L = int(np.max(stk_len))
    logits, _, cache = MR.multi_speller_fwd(tiled, tiled_lens, stk_targets[:, :L], stk_len, p, attention)
    loss, _, _, dlogits = mwer_ref.loss_grad(logits, stk_targets, stk_len, errors, valid, CE_WEIGHT, 1.0 / B)
    dtiled, grads = MR.multi_speller_bwd(dlogits, cache)
    return float(loss.sum() / B), [mwer_ref.tile_bwd(d, R) for d in dtiled], grads
