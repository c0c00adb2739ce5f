"""CPU: every committed seed of tests/mwer_cases.py leaves the float64 N-best a margin float32 cannot close, and the
float64 chain of the end-to-end test is the gradient of its own loss."""
import numpy as np
import pytest

from tests import beam_joint_cases as J
from tests import mwer_cases as MC
from tests import mwer_ref


@pytest.mark.parametrize('kind', MC.KINDS)
def test_committed_seeds_have_a_margin(kind):
    beams, gap, T = MC.brute_force(kind)
    assert gap >= J.MARGIN
    assert T == J.SEARCH['S'] and all(len(utt) == MC.N for utt in beams)
    assert all(utt[k][2] >= utt[k + 1][2] for utt in beams for k in range(MC.N - 1))       # best first


def test_float64_chain_is_the_gradient_of_its_loss(monkeypatch):
    kind = 'vanilla'
    attention, p, encs, enc_lens, targets, target_len = MC.case(kind)
    beams, _, _ = MC.brute_force(kind)
    B, S = J.SEARCH['B'], J.SEARCH['S']
    seq = np.zeros((B, MC.N, S), np.int32)
    lengths = np.zeros((B, MC.N), np.int32)
    for b, utt in enumerate(beams):
        for n, (labels, length, _) in enumerate(utt):
            seq[b, n, :length], lengths[b, n] = labels, length
    stk, stk_len, hyp_len, valid = mwer_ref.prepare(seq, lengths, np.zeros((B, MC.N), np.float32), targets, target_len,
                                                    J.SEARCH['C'])
    errs = mwer_ref.errors(stk, hyp_len, targets, target_len)
    assert len(set(errs.reshape(MC.N, B)[:, 0])) > 1 or len(set(errs.reshape(MC.N, B)[:, 2])) > 1
    loss, dencs, _ = MC.float64_chain(kind, stk, stk_len, errs, valid)
    # central differences along a random direction of the encoded input
    rng = np.random.default_rng(3)
    direction = rng.normal(size=encs[0].shape) * (np.arange(encs[0].shape[1])[None, :, None] < enc_lens[0][:, None, None])
    h = 1e-5
    keep = J.search_case

    def shifted(sign):
        def case(k, s):
            a, pp, e, l, c = keep(k, s)
            return a, pp, [e[0].astype(np.float64) + sign * h * direction] + list(e[1:]), l, c
        return case
    monkeypatch.setattr(J, 'search_case', shifted(+1))
    up = MC.float64_chain(kind, stk, stk_len, errs, valid)[0]
    monkeypatch.setattr(J, 'search_case', shifted(-1))
    down = MC.float64_chain(kind, stk, stk_len, errs, valid)[0]
    monkeypatch.setattr(J, 'search_case', keep)
    want = (up - down) / (2 * h)
    got = float((dencs[0] * direction).sum())
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want)
