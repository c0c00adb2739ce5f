"""CTC beam-search cases for the limits of decode.hip and their admissibility (plain NumPy; importable without a GPU).

The kernel keeps its beam in float32, the oracle (oracle.decode_oracle.ctc_beam_search) in float64.  The two can be
held to the SAME labelling only where no decision of the search hangs on less than float32 can resolve, so every case
here is built from a seed that a CPU search (find_seeds, at the bottom) has accepted: the oracle alone, run with
details=True, must show margins above guard_bound().  tests/test_decode_cases.py asserts that for every committed
seed without a GPU; tests/test_hip_decode_limits.py asserts it again before it touches the device.

  guard_bound   4 T eps32 max(1, max|total|): one float32 rounding of a total per frame on the blank path and one on
                the label path, doubled.  select_gap (the threshold of every selection), top_gap (the winner) and, in
                the cases built to tie, order_gap (the order of the kept beam decides which of two tied candidates has
                the lower index) must exceed it.
  lp_bound      2 T eps32 max(1, |total|): what the returned log-probability may differ from the oracle's total."""
import numpy as np

from oracle import decode_oracle as D

EPS32 = float(np.finfo(np.float32).eps)


def guard_bound(T, det):
    return 4.0 * T * EPS32 * max(1.0, det['max_abs_total'])


def lp_bound(T, total):
    return 2.0 * T * EPS32 * max(1.0, abs(float(total)))


def inadmissible(det, T, ties=False):
    """None if the oracle's run `det` (details=True, T frames) leaves float32 no decision to get wrong, else why not.
    Exact ties at a selection threshold are admitted only with ties=True (cases built to tie), which also holds the
    order inside the kept beams to the bound."""
    g = guard_bound(T, det)
    if not det['select_gap'] > g:
        return 'select_gap %.3g <= %.3g' % (det['select_gap'], g)
    if not det['top_gap'] > g:
        return 'top_gap %.3g <= %.3g' % (det['top_gap'], g)
    if det['select_ties'] and not ties:
        return '%d exact ties at a selection threshold' % det['select_ties']
    if ties and not det['order_gap'] > g:
        return 'order_gap %.3g <= %.3g' % (det['order_gap'], g)
    return None


def oracle(logits, lens, W, merge=True):
    """details of every utterance; lengths are clamped to [0, T] as the kernel clamps them"""
    T = logits.shape[1]
    return D.ctc_decode_batch(logits, np.clip(lens, 0, T), W, merge, details=True)


# ---------------------------------------------------------------------------------------------------------------
# case 1: the W-th survivor decides.  Early frames flat, late frames peaked.
def random_width_logits(C, T, seed):
    """beams narrower than the alphabet (the threshold cuts the single labels of frame 0): N(0, 0.3) on the first half
    of the frames, N(0, 3) on the second"""
    rng = np.random.default_rng([seed, C, T])
    sigma = np.where(np.arange(T) < (T + 1) // 2, 0.3, 3.0)
    return (sigma[:, None] * rng.standard_normal((T, C))).astype(np.float32)


ALPHA, BETA, KAPPA, PEAK, BLANK_PEAK = 2e-4, 8e-3, 0.5, 4.0, 8.0


def staircase_logits(W, C, T, seed):
    """beams of C - 1 <= W < (C - 1) (C - 2): the threshold of frame 1 cuts through the two-label prefixes.

    A random order r of the labels.  Frame 0 leans against r by ALPHA per rank, frame 1 with r by BETA per rank, the
    blank has probability ~KAPPA / C in both: the two-label prefixes 'x y' (mass p0(x) p1(y), all within a few per
    cent of each other) then rank by r(y) descending and, inside a family of equal y, by r(x) ascending, below the
    single labels.  The beam cuts one family y* after its k-th member.  Frame 2 is peaked on y*: 'u y*' collects the
    mass of its parent 'u' — which GROWS with r(u) — on top of its own if it was kept, and the spread of the parents
    over the family is smaller than a pair's own mass; so the LAST KEPT member of the family ends up the most
    probable prefix: one member later with W + 1, one earlier with W - 1.  The remaining frames are peaked on the
    blank.  A little seeded noise moves the margins; the search keeps the seeds at which every one is wide enough."""
    assert T >= 3 and C - 1 <= W < (C - 1) * (C - 2)
    rng = np.random.default_rng([seed, W, C, T])
    r = rng.permutation(C - 1).astype(np.float64)
    x = np.zeros((T, C))
    x[0, :C - 1] = -ALPHA * r
    x[1, :C - 1] = BETA * r
    x[:2, C - 1] = np.log(KAPPA)
    x[:2, :C - 1] += 0.1 * ALPHA * rng.standard_normal((2, C - 1))
    early = np.ascontiguousarray(x[:2], np.float32)
    cut = D.ctc_beam_search(early, 1 << 30, False, details=True)['beam'][W - 1][0]
    assert len(cut) == 2, cut
    x[2:] = 0.05 * rng.standard_normal((T - 2, C))
    x[2, cut[1]] += PEAK
    x[3:, C - 1] += BLANK_PEAK
    x[:2] = early
    return x.astype(np.float32)


def width_case(W, C, T, seeds):
    """[B, T, C] logits, one utterance per seed"""
    make = staircase_logits if W >= C - 1 else (lambda W, C, T, s: random_width_logits(C, T, s))
    return np.stack([make(W, C, T, s) for s in seeds])


def width_decides(x, W, merge=True):
    """(details at W, labelling at W - 1 or None, labelling at W + 1) of one utterance [T, C]"""
    det = D.ctc_beam_search(x, W, merge, details=True)
    below = D.ctc_beam_search(x, W - 1, merge) if W > 1 else None
    return det, below, D.ctc_beam_search(x, W + 1, merge)


def width_ok(x, W):
    T = x.shape[0]
    det, below, above = width_decides(x, W)
    if det['labels'] == below or det['labels'] == above:
        return False
    # the neighbouring widths are decisions of the oracle too: hold them to the same margins
    return all(inadmissible(D.ctc_beam_search(x, w, True, details=True), T) is None for w in (W - 1, W, W + 1) if w)


# (W, C, T, seeds): found by find_seeds(lambda s: width_ok(width_case(W, C, T, [s])[0], W), 2)
WIDTH_CASES = [
    (1, 5, 6, (1, 4)), (2, 5, 6, (4, 7)), (8, 5, 6, (0, 1)), (100, 40, 6, (0, 1)), (256, 40, 6, (0, 1)),
]


# ---------------------------------------------------------------------------------------------------------------
# case 6: structural ties at the threshold in a non-uniform setting.  Classes 1 and 2 share bit-identical columns,
# so 'p 1' and 'p 2' tie exactly for every prefix p while the other candidates lie above and below.
TIE_A, TIE_B = 1, 2


def tie_logits(C, T, seed):
    rng = np.random.default_rng([seed, C, T, 6])
    x = (1.5 * rng.standard_normal((T, C))).astype(np.float32)
    x[:, TIE_B] = x[:, TIE_A]
    return x


def tie_ok(x, W):
    """the beam cuts through a tied group, nothing else is close, and the winner contains one of the twin classes:
    its mirror image (1 <-> 2) has the same total wherever both are alive, so with top_gap > 0 the mirror image was
    cut off at a tie — under the opposite tie rule the mirror image would have won"""
    det = D.ctc_beam_search(x, W, True, details=True)
    return (det['select_ties'] > 0 and inadmissible(det, x.shape[0], ties=True) is None
            and (TIE_A in det['labels'] or TIE_B in det['labels']))


# (C, T, W, seeds): W = 7 is one of the widths at which find_seeds(lambda s: tie_ok(tie_logits(C, T, s), W), 2) succeeds
TIE_CASE = (6, 5, 7, (0, 31))


# ---------------------------------------------------------------------------------------------------------------
# the other cases: seeded normal logits, the seed only has to be admissible
def normal_logits(B, T, C, seed, sigma=1.0):
    return (sigma * np.random.default_rng([seed, B, T, C]).standard_normal((B, T, C))).astype(np.float32)


def all_admissible(logits, lens, W, merges=(True,)):
    T = logits.shape[1]
    return all(inadmissible(d, int(np.clip(n, 0, T))) is None
               for m in merges for d, n in zip(oracle(logits, lens, W, m), lens))


NEG = -np.inf


def plain_case(name, seed):
    """(logits [B,T,C], lens [B], W, merge settings) of the cases that need nothing but an admissible seed"""
    if name == 'max_width':             # 98 464 bytes of LDS; the beam is full from frame 2: 10 240 keys per selection
        return normal_logits(3, 6, 40, seed), np.array([6, 6, 4], np.int32), 256, (True,)
    if name == 'one_label':             # C = 2
        return normal_logits(3, 9, 2, seed), np.array([9, 9, 5], np.int32), 4, (True, False)
    if name == 'lengths':               # 1, T and T + 5 (clamped to T)
        return normal_logits(3, 7, 5, seed), np.array([1, 7, 12], np.int32), 4, (True,)
    assert name == 'neg_inf'
    x = normal_logits(4, 6, 5, seed)
    x[0, 1, 0] = x[0, 3, 0] = x[0, 3, 1] = x[0, 4, 2] = NEG     # label classes at -inf on some frames
    x[1, 2, :4] = NEG                                           # a frame where only the blank is finite
    x[2, 3, 4] = NEG                                            # a frame where the blank is -inf
    x[3, 3, :] = NEG                                            # a frame without a log-softmax: every candidate dies
    return x, np.array([6, 6, 6, 6], np.int32), 4, (True,)


# name -> seed: find_seeds(lambda s: all_admissible(*plain_case(name, s)))
PLAIN_CASES = {'max_width': 0, 'one_label': 0, 'lengths': 0, 'neg_inf': 0}


def find_seeds(ok, count=1, start=0, stop=100000):
    """the first `count` seeds in [start, stop) that `ok` accepts — run by hand when a case is added; its results are
    written into the tables of this file, and tests/test_decode_cases.py holds them to `ok` again"""
    found = []
    for seed in range(start, stop):
        if ok(seed):
            found.append(seed)
            if len(found) == count:
                return found
    raise LookupError('no %d seeds in [%d, %d): %r' % (count, start, stop, found))
