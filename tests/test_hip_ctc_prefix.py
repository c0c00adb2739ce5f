"""nabu_ctc_prefix_prepare / _score / _advance (ctc_prefix.hip) on their own against float64 (tests/ctc_prefix_ref.py,
itself held to an enumeration of all paths by tests/test_ctc_prefix_ref.py).

The yardstick is that of tests/ctc_cases.py: judge — a kernel's error against float64 may be K times the error of the
float32 restatement on the same case plus a floor.  Errors are taken relative to max(1, |log-probability|) (for a
delta: the larger of the two psi it is the difference of).  K = 4 for the state and the deltas (maxima over many
entries), K_NLL = 16 for psi [B,W] (a handful of single log-probabilities, each the end of a T-step chain).  The floor
is 8 * 2^-24: at T = 1 a result is (x - max) - log(sum exp), two library calls which the device's libm delivers to
1-2 ulp where NumPy's are within 0.5 ulp, one subtraction and the sum — the float32 restatement can be exact there.
Every case chains three steps of hand-chosen parent / stay / pred, so states are inherited; the kernel's chain, the
float32 chain and the float64 chain each start from their own previous state.

Measured on the MI355X (LABNOTES.md section 30): no case needs a multiple beyond the floor except the state at
W 1, C 40, T 125 with a chain of dependent log-sum-exps per frame (0.09); with the scans and sums the kernels run now
every quantity stays inside the floor, so the multiples needed are 0.  Without the floor, the kernels' errors are
0.6 to 2.0 times the float32 restatement's (worst: psi at W 5, C 3, T 7: 4.0 against 2.0 units of 2^-24; the
normalisers at W 3, C 300, T 125: 5.1 against 3.0), and at most 5.3 units of 2^-24 relative to the log-probability.
`python -m pytest tests/test_hip_ctc_prefix.py -s` prints the table."""
import numpy as np
import pytest
import torch

from nabu_amd import _hip, ops
from tests import ctc_prefix_ref as R
from tests.ctc_cases import K, K_NLL, U

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 8 * U
DEAD = -1e29


def t(a):
    return torch.tensor(a, device=DEV)


def lengths_for(T):
    """ragged: full, half, and one shorter than the three-label hypotheses of the plan (T = 1: an empty utterance)"""
    return np.array([T, max(1, T // 2), min(T, 2) if T > 1 else 0], np.int32)


def plan(step, W, C, last, finished):
    """hand-chosen survivors of step 0, 1, 2 from the beam's last labels and finished flags: (parent, stay, pred) [W]"""
    eos, k = C - 1, np.arange(W)
    if step == 0:       # every slot extends the empty hypothesis (slot 0) by its own label; the last slot ends
        parent = np.zeros(W, np.int32)
        pred = (k % (C - 1)).astype(np.int32)
        if W > 1:
            pred[W - 1] = eos
    elif step == 1:     # every slot goes on from itself: even slots REPEAT their last label, odd ones take the next
        parent = k.astype(np.int32)
        pred = np.where(k % 2 == 0, last, (last + 1) % (C - 1)).astype(np.int32)
    else:               # inherit from the neighbour: repeat again / end / another label
        parent = ((k + 1) % W).astype(np.int32)
        pl = last[parent]
        pred = np.where(k % 3 == 0, pl, np.where(k % 3 == 1, eos, (pl + 2) % (C - 1))).astype(np.int32)
    stay = finished[parent].astype(np.int32)
    pred = np.where(stay > 0, eos, pred).astype(np.int32)
    return parent, stay, pred


def judge(what, got, r64, r32, k, scale=None, worst=None):
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    assert np.all(np.isfinite(got)), '%s: not finite' % what
    dead = r64 <= DEAD
    assert np.all(got[dead] <= DEAD), '%s: log 0 expected' % what
    assert np.all(got[~dead] > DEAD), '%s: unexpected log 0' % what
    if dead.all():
        return
    s = np.maximum(1.0, np.abs(r64) if scale is None else scale)[~dead]
    e_ker = float((np.abs(got - r64)[~dead] / s).max())
    e_ref = float((np.abs(r32 - r64)[~dead] / s).max())
    need = max(e_ker - FLOOR, 0.0) / e_ref if e_ref > 0 else (0.0 if e_ker <= FLOOR else float('inf'))
    if worst is not None:       # per quantity: (multiple needed beyond the floor, error in units of 2^-24, the restatement's)
        key = what.split(' ')[0]
        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0, 0.0)), (need, e_ker / U, e_ref / U)))
    assert e_ker <= k * e_ref + FLOOR, '%s: e_ker %.3e > %g * e_ref %.3e + 8u (needs %.2f)' % (what, e_ker, k, e_ref, need)


def judge_beam(what, s, b64, b32, worst):
    judge('state ' + what, s.state.cpu().numpy(), b64['state'], b32['state'], K, worst=worst)
    judge('psi ' + what, s.psi.cpu().numpy(), b64['psi'], b32['psi'], K_NLL, worst=worst)
    np.testing.assert_array_equal(s.last.cpu().numpy(), b64['last'])


def judge_delta(what, delta, beam64, d64, d32, finished, worst):
    live = finished == 0
    psi_g = beam64['psi'][:, :, None]
    scale = np.maximum(np.abs(psi_g), np.abs(np.maximum(d64 + psi_g, R.NEG)))
    scale = np.where(scale > -DEAD, 1.0, scale)
    judge('delta ' + what, delta[live], d64[live], d32[live], K, scale=np.broadcast_to(scale, d64.shape)[live], worst=worst)
    assert np.all(delta[~live] == 0), '%s: the row of a finished beam is zero' % what


CASES = [
    # (W, C, T, sigma)
    (5, 3, 7, 1.0),        # more beams than classes; a single partial wave
    (5, 3, 125, 8.0),
    (5, 3, 2, 1.0),
    (5, 3, 1, 8.0),
    (1, 40, 125, 1.0),     # W = 1; the recipe's class count and frame count
    (4, 40, 125, 8.0),     # peaked posteriors
    (2, 40, 2, 8.0),
    (2, 40, 1, 1.0),
    (3, 300, 7, 1.0),      # more classes than a block
    (3, 300, 125, 8.0),
    (3, 65, 9, 1.0),       # the first class count of a 128-thread block; T = 9: one frame behind the look-ahead of 8
]


@pytest.mark.parametrize('W,C,T,sigma', CASES, ids=['W%d-C%d-T%d-s%g' % c for c in CASES])
def test_prepare_score_advance_chain_against_float64(W, C, T, sigma):
    B = 3
    rng = np.random.default_rng([W, C, T, int(sigma)])
    logits = (sigma * rng.standard_normal((B, T, C))).astype(np.float32)
    enc_len = lengths_for(T)
    worst = {}
    y64, b64 = R.prepare(logits, enc_len, W, np.float64)
    y32, b32 = R.prepare(logits, enc_len, W, np.float32)
    s = ops.ctc_prefix_prepare(t(logits), t(enc_len), W)
    # the normalisers: y = (x - mx) - lz
    norm = s.norm.cpu().numpy()
    valid = np.arange(T)[None, :] < enc_len[:, None]
    y_ker = (logits - norm[:, :, :1]) - norm[:, :, 1:]
    judge('norm', y_ker[valid], y64[valid], y32[valid], K, worst=worst)
    judge_beam('of the empty hypothesis', s, b64, b32, worst)
    finished = np.zeros((B, W), np.int32)
    for step in range(3):
        d64, d32 = R.score(y64, enc_len, b64, finished), R.score(y32, enc_len, b32, finished)
        fin_d = t(finished)
        delta = ops.ctc_prefix_score(s, fin_d)
        judge_delta('step %d' % step, delta.cpu().numpy(), b64, d64, d32, finished, worst)
        if finished.any():      # a finished beam's state is not read: poison it
            poisoned = ops.CtcPrefixState(s.logits, s.enc_len, s.norm, W, s.state.clone(), s.psi.clone(), s.last)
            poisoned.state[fin_d.bool()] = float('nan')
            poisoned.psi[fin_d.bool()] = float('nan')
            assert torch.equal(ops.ctc_prefix_score(poisoned, fin_d), delta)
        moves = [plan(step, W, C, b64['last'][b], finished[b]) for b in range(B)]
        parent, stay, pred = (np.stack([m[i] for m in moves]) for i in range(3))
        b64, b32 = R.advance(y64, enc_len, b64, parent, stay, pred), R.advance(y32, enc_len, b32, parent, stay, pred)
        old = s.state.clone()
        s, prev = ops.ctc_prefix_advance(s, t(parent), t(stay), t(pred)), s
        assert torch.equal(prev.state, old)                    # the old state is left as it was
        judge_beam('after step %d' % step, s, b64, b32, worst)
        finished = (pred == C - 1).astype(np.int32)
    # the utterance shorter than its hypotheses: every live three-label hypothesis of it scores log 0
    if T > 1:
        live = (finished[2] == 0) & (b64['last'][2] >= 0)
        assert np.all(b64['psi'][2][live] <= DEAD) and (live.any() or W == 2)
    print('W%d C%d T%d sigma%g (multiple needed, error / 2^-24, float32 restatement / 2^-24): %s'
          % (W, C, T, sigma, ', '.join('%s %.2f %.2f %.2f' % ((k,) + v) for k, v in sorted(worst.items()))))


def test_refusals_come_from_the_host():
    """4 T floats of LDS for the score kernel: T = 10241 needs 163 856 bytes, more than a workgroup has"""
    B, W, C, T = 1, 1, 3, 10241
    assert 4 * T * 4 == 163856 > 160 * 1024
    logits = torch.zeros((B, T, C), device=DEV)
    s = ops.CtcPrefixState(logits, t(np.array([T], np.int32)), torch.zeros((B, T, 2), device=DEV), W)
    with pytest.raises(_hip.NabuHipError, match='LDS'):
        ops.ctc_prefix_score(s, t(np.zeros((B, W), np.int32)))
    # and a valid call works afterwards
    small = ops.ctc_prefix_prepare(t(np.zeros((1, 2, 3), np.float32)), t(np.array([2], np.int32)), 1)
    assert small.psi.cpu().numpy()[0, 0] == 0
