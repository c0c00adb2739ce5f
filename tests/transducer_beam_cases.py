"""Inputs of the beam-search tests (importable without a GPU), all on the quarter grid so that every joint logit is
exact in float32.

beam_inputs(C, seed): f [5,6,C], enc_len = [T, T-1, 0, 1, T+3] and g_fn(b, labels) for S = 4.
  A frame's labels take 0, -1, -2, .. by a random permutation (the first 16; the rest -20) and the blank 1: the blank
  is raised, and no two classes of a frame are equal among those a beam of 8 can select.  The prediction logits of a
  history are 0, 1/4, 1/2 or 3/4 per class, drawn from (seed, b, labels): less than the spacing of a frame, so they
  never make two classes of a hypothesis equal, and different histories get different normalisers.
  utterance 0  the planted merge: on frames 0 and 1 the blank has 3/4, label 0 has 0, label 1 has -1 and the others
               -4 and less; a history that begins with 0 puts 8 on the blank, and so do all later frames;
               the prediction logits of label 0 and the blank are 0 otherwise.  p(()) is
               about 0.37, the two alignments of (0) have 0.29 and 0.17: each loses to () and together they win;
  utterance 1  enc_len = T-1, f is NaN from there on;
  utterance 2  enc_len = 0: f is NaN throughout;
  utterance 3  enc_len = 1, f is NaN from frame 1 on;
  utterance 4  enc_len = T+3 (the clamp); label 0 has 3 on every frame: the best hypothesis reaches S labels at once
               and goes on through blanks."""
import numpy as np

B, T, S = 5, 6, 4
SEEDS = {3: 3, 5: 4, 70: 3}            # per C: chosen on the CPU (tests/test_transducer_beam_ref.py checks the conditions)


def _frame(rng, C, base=0.0):
    x = np.full(C, -20.0)
    rank = rng.permutation(C - 1)
    x[:C - 1] = np.where(rank < 16, base - rank, -20.0)
    x[C - 1] = 1.0
    return x


def beam_inputs(C, seed=None):
    seed = SEEDS.get(C, 1) if seed is None else seed
    rng = np.random.default_rng([seed, C])
    f = np.stack([np.stack([_frame(rng, C) for _ in range(T)]) for _ in range(B)])
    enc_len = np.array([T, T - 1, 0, 1, T + 3], np.int32)
    for t in range(T):                                   # utterance 0
        if t < 2:
            x = _frame(rng, C, -4.0)
            x[0] = 0.0
            x[1] = -1.0
            x[C - 1] = 0.75
            f[0, t] = x
        else:
            f[0, t, C - 1] = 8.0
    f[4, :, 0] = 3.0
    f[1, T - 1:] = np.nan
    f[2] = np.nan
    f[3, 1:] = np.nan

    def g_fn(b, y):
        y = tuple(int(k) for k in y)
        g = np.random.default_rng([seed, C, b, len(y)] + list(y)).integers(0, 4, C) / 4.0
        if b == 0:
            g[[0, C - 1]] = 0.0
            if y and y[0] == 0:
                g[C - 1] = 8.0
        return g
    return f, enc_len, g_fn


def conditions(res, plain, W):
    """what the step-by-step comparison needs of the restatement's run `res` (and of `plain`, the run without the
    merge) to be a fair and a telling demand; a list of the conditions that FAIL"""
    bad = []
    if not res['margin'] >= 1e-3:
        bad.append('smallest selection margin %.3e < 1e-3' % res['margin'])
    if not any(res['capped']):
        bad.append('no hypothesis reaches S and continues by blanks')
    if not any(res['shrinks']):
        bad.append('no iteration shrinks the beam')
    if W >= 2:                    # (a beam of one holds no pair to merge, and one final is all it can keep)
        if not any(res['merges']):
            bad.append('no merge')
        if not any(a[0][0] != b[0][0] for a, b in zip(res['finals'], plain['finals'])):
            bad.append('the best final is the same with and without the merge in every utterance')
        if not any(len(fin) < W for fin in res['finals']):
            bad.append('every utterance ends with W finals')
    return bad
