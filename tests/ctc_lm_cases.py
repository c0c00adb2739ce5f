"""Cases of the CTC beam search with a label n-gram (nabu_ctc_beam_search_lm) and their admissibility (plain NumPy;
importable without a GPU).  As in tests/decode_cases.py the float32 kernel can be held to the float64 reference's
labelling only where no decision hangs on less than float32 resolves: every case is built from a committed seed at
which the reference alone (tests/ctc_lm_ref.py, details=True) shows select_gap and top_gap above
decode_cases.guard_bound and no exact tie.  tests/test_ctc_lm_cases.py asserts that on the CPU,
tests/test_hip_ctc_lm.py again before it touches the device.  Seeds were found with decode_cases.find_seeds."""
import numpy as np

from tests import ctc_lm_ref as R
from tests import decode_cases as DC
from tests import ngram_lm_ref as NR

ALPHA, BETA = 0.8, 0.5


def admissible(dets, lens, T):
    return all(DC.inadmissible(d, max(1, int(np.clip(n, 0, T)))) is None for d, n in zip(dets, lens))


# ---------------------------------------------------------------------------------------------------------------
# parity: (name, B, T, C, lens, W, order, merge)
def _parity():
    out = []
    for W in (1, 4, 100):                       # 100 exceeds the candidates of the early frames
        for order in (1, 2, 3):
            for merge in (True, False):
                out.append(('small-W%d-n%d-%s' % (W, order, 'merge' if merge else 'keep'), 3, 12, 5, (12, 1, 0), W, order, merge))
    for merge in (True, False):                 # one label: the C-1 index arithmetic degenerates
        out.append(('one_label-%s' % ('merge' if merge else 'keep'), 3, 9, 2, (9, 5, 0), 4, 3, merge))
    out.append(('recipe', 2, 20, 41, (20, 13), 100, 3, True))       # the recipe's alphabet
    return out


PARITY = _parity()


def parity_case(case, seed):
    """(logits [B,T,C] float32, lens int32 [B], table float32)"""
    name, B, T, C, lens, W, order, merge = case
    return DC.normal_logits(B, T, C, seed, sigma=1.5), np.array(lens, np.int32), NR.random_table(C, order, seed)


def parity_reference(case, seed):
    name, B, T, C, lens, W, order, merge = case
    logits, lens, table = parity_case(case, seed)
    return R.search_batch(logits, lens, table, order, ALPHA, BETA, W, merge)


def parity_ok(case, seed):
    return admissible(parity_reference(case, seed), case[4], case[2])


# name -> seed: find_seeds(lambda s: parity_ok(case, s))
PARITY_SEEDS = dict({c[0]: 0 for c in PARITY}, recipe=1)


# ---------------------------------------------------------------------------------------------------------------
# the self loop: logits peaked along a frame path in which label 0 is held over several frames.  A search that added
# the term on the repeated-label self loop as well (ctc_lm_ref.search(term_on_self_loop=True)) must pick another winner.
SELF_ALPHA, SELF_C, SELF_W = 1.5, 3, 8
SELF_PATHS = {'blank_between': ((0, 0, 2, 0, 0, 2), False),      # 'a a _ a a _' -> [a, a]   (merge_repeated off: kept)
              'true_repeat': ((0, 0, 0, 1, 1, 2), True)}          # 'a a a b b _' -> [a, b]


def self_loop_case(name, seed):
    path, merge = SELF_PATHS[name]
    T = len(path)
    rng = np.random.default_rng([seed, T, 11])
    x = rng.standard_normal((1, T, SELF_C))
    x[0, np.arange(T), path] += 3.0
    return x.astype(np.float32), np.array([T], np.int32), NR.random_table(SELF_C, 2, seed, sharp=2.0), merge


def self_loop_reference(name, seed):
    """(details of the search, labels of the wrong variant)"""
    logits, lens, table, merge = self_loop_case(name, seed)
    det = R.search(logits[0], table, 2, SELF_ALPHA, 0.0, SELF_W, merge, details=True)
    wrong = R.search(logits[0], table, 2, SELF_ALPHA, 0.0, SELF_W, merge, details=True, term_on_self_loop=True)
    return det, wrong


def self_loop_ok(name, seed):
    path, merge = SELF_PATHS[name]
    det, wrong = self_loop_reference(name, seed)
    want = [0, 0] if name == 'blank_between' else [0, 1]
    return (det['labels'] == want and wrong['labels'] != det['labels']
            and DC.inadmissible(det, len(path)) is None and DC.inadmissible(wrong, len(path)) is None)


SELF_SEEDS = {'blank_between': 11, 'true_repeat': 3}


# ---------------------------------------------------------------------------------------------------------------
# the LM matters: the plain and the fused winners differ
MATTERS = dict(B=2, T=8, C=5, W=8, order=2, alpha=1.5, beta=0.0)


def matters_case(seed):
    m = MATTERS
    return (DC.normal_logits(m['B'], m['T'], m['C'], seed), np.array([m['T']] * m['B'], np.int32),
            NR.random_table(m['C'], m['order'], seed, sharp=2.0))


def matters_reference(seed):
    m = MATTERS
    logits, lens, table = matters_case(seed)
    fused = R.search_batch(logits, lens, table, m['order'], m['alpha'], m['beta'], m['W'], True)
    plain = R.search_batch(logits, lens, table, m['order'], 0.0, 0.0, m['W'], True)
    return fused, plain


def matters_ok(seed):
    fused, plain = matters_reference(seed)
    lens = [MATTERS['T']] * MATTERS['B']
    return (admissible(fused, lens, MATTERS['T']) and admissible(plain, lens, MATTERS['T'])
            and all(f['labels'] != p['labels'] for f, p in zip(fused, plain)))


MATTERS_SEED = 0

# identity at alpha = beta = 0: two committed cases of tests/decode_cases.py (name, order of the table that is ignored)
IDENTITY = (('lengths', 2), ('max_width', 1))
