"""nabu_transducer_loss_grad and nabu_transducer_greedy_step (csrc/transducer.hip) against the float64 restatement of
tests/transducer_ref.py, by the yardstick of tests/transducer_cases.py (judge: ctc_cases' K = 4 / K_NLL = 16 times what
the float32 run of the restatement loses on the same case).

In this process the default dispatch runs (the wave route for U1 <= 64); ONE child process runs those shapes with
NABU_TRANSDUCER_WORKGROUP=1 and the parent compares bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import transducer_cases as tc
from tests import transducer_check as ck
from tests import transducer_ref as tr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_default = {}          # entry id -> (nll, df, dg, status) of the default dispatch (computed once)


def _default_run(entry):
    key = ck.entry_id(entry)
    if key not in _default:
        _default[key] = ck.run(ck.case_of(entry))
    return _default[key]


def _judged(out, case, what, grad_scale=1.0):
    v = tc.judge(out[0], out[1], out[2], case, grad_scale)
    print(what, 'needed (grad, sums, nll) = %.2f %.2f %.2f' % tc.needed(v, case),
          'errors %.3e / %.3e, %.3e / %.3e, %.3e / %.3e' % (v.e_ker, v.e_ref, v.s_ker, v.s_ref, v.n_ker, v.n_ref))
    return v


def _rows_past_the_lengths_are_zero(case, df, dg):
    for b in range(len(case.enc_len)):
        assert np.all(df[b, case.enc_len[b]:] == 0) and np.all(dg[b, case.label_len[b] + 1:] == 0), b


@pytest.mark.parametrize('entry', ck.ENTRIES, ids=[ck.entry_id(e) for e in ck.ENTRIES])
def test_loss_and_gradients_within_the_yardstick(entry):
    """nll, df, dg and the row sums by judge(); zero rows past the lengths; a second call gives the same bits"""
    assert not ck.forced_workgroup(), 'NABU_TRANSDUCER_WORKGROUP is set: this test would not reach the wave route'
    case = ck.case_of(entry)
    out = _default_run(entry)
    nll, df, dg, status = out
    assert status == 0 and nll.dtype == df.dtype == dg.dtype == np.float32
    v = _judged(out, case, ck.entry_id(entry))
    assert v.ok, v.report
    _rows_past_the_lengths_are_zero(case, df, dg)
    again = ck.run(case)
    assert again[3] == 0 and ck.same_bits(again[:3], out[:3]), 'second call differs from the first'


def test_grad_scale():
    entry = ((3, 12, 65, 6), 'random')
    for scale in (1.0 / 3, 0.37):
        out = ck.run(ck.case_of(entry), scale)
        v = _judged(out, ck.case_of(entry), 'scale %g' % scale, scale)
        assert v.ok, v.report


def test_workgroup_route_on_the_wave_routes_shapes(tmp_path):
    """the switch is read once per process: a fresh child runs every shape with U1 <= 64 on the workgroup route; nll,
    df and dg must be the default dispatch's, bit for bit"""
    todo = [e for e in ck.ENTRIES if tc.wave_eligible(e[0][3])]
    assert len(todo) == 3 * 11
    path = str(tmp_path / 'forced.npz')
    e = dict(os.environ)
    e['NABU_TRANSDUCER_WORKGROUP'] = '1'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'transducer_check.py'), path], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'TRANSDUCER DONE' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    with np.load(path) as forced:
        for entry in todo:
            key = ck.entry_id(entry)
            out = _default_run(entry)
            assert int(forced[key + '/status']) == out[3] == 0, key
            for name, a in zip(('nll', 'df', 'dg'), out[:3]):
                assert ck.same_bits([a], [forced['%s/%s' % (key, name)]]), '%s: %s differs between the routes' % (key, name)


SHIFTED = [(s, r) for s in [(3, 12, 65, 6), (4, 70, 40, 63), (2, 40, 12, 256)] for r in ('random', 'peaky')]


@pytest.mark.parametrize('entry', SHIFTED, ids=[ck.entry_id(e) for e in SHIFTED])
def test_shift_invariance(entry):
    """+80 or -80 on every row of f and of g (tc.shift_case: exact in float32, so every joint logit is the unshifted
    one plus a constant per node): nll, df and dg stay within judge() of the UNSHIFTED float64 values, with the
    unshifted float32 run as the measure.  A peak of f and a peak of g on different classes are 160 + apart here: the
    product exp(f - max f) exp(g - max g) would underflow."""
    moved, plain = tc.shift_case(ck.case_of(entry), tc.seed_of(*entry[0]))
    out = ck.run(moved)
    assert out[3] == 0
    v = _judged(out, plain, 'shifted ' + ck.entry_id(entry))
    assert v.ok, v.report
    base = ck.run(plain)
    assert _judged(base, plain, 'on the grid ' + ck.entry_id(entry)).ok


def _raw_call(case, fill, ws_less=0, **over):
    """nabu_transducer_loss_grad on outputs pre-filled with `fill`; returns (rc, nll, df, dg, status)"""
    import torch
    from nabu_amd import _hip
    f, g, enc_len, labels, label_len = case
    B, T, C = f.shape
    U1 = g.shape[1]

    def dev(a, dtype):
        return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()
    fd, gd, el, ll = dev(f, torch.float32), dev(g, torch.float32), dev(enc_len, torch.int32), dev(label_len, torch.int32)
    lab = dev(labels, torch.int32)
    nll = torch.full((B,), fill, dtype=torch.float32, device='cuda')
    df, dg = torch.full_like(fd, fill), torch.full_like(gd, fill)
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    L = _hip.lib()
    wsb = L.nabu_transducer_ws_bytes(B, T, U1)
    ws = torch.full((wsb // 4 + 4,), float('nan'), dtype=torch.float32, device='cuda')     # a workspace full of NaN
    a = dict(B=B, T=T, U1=U1, C=C, f=_hip.ptr(fd), g=_hip.ptr(gd), el=_hip.ptr(el), lab=_hip.ptr(lab), ldl=labels.shape[1],
             ll=_hip.ptr(ll), nll=_hip.ptr(nll), df=_hip.ptr(df), dg=_hip.ptr(dg), status=_hip.ptr(status), ws=_hip.ptr(ws))
    a.update(over)
    rc = L.nabu_transducer_loss_grad(a['B'], a['T'], a['U1'], a['C'], a['f'], a['g'], a['el'], a['lab'], a['ldl'], a['ll'], 1.0,
                                     a['nll'], a['df'], a['dg'], a['status'], a['ws'], wsb - ws_less, _hip.stream())
    torch.cuda.synchronize()
    return rc, nll.cpu().numpy(), df.cpu().numpy(), dg.cpu().numpy(), int(status.item()), L.nabu_last_error()


@pytest.mark.parametrize('shape', [(3, 12, 65, 6), (4, 70, 40, 64)], ids=str)
def test_outputs_and_workspace_prefilled_with_nan(shape):
    case = ck.case_of((shape, 'random'))
    rc, nll, df, dg, status, _ = _raw_call(case, float('nan'))
    assert rc == 0 and status == 0
    assert np.all(np.isfinite(nll)) and np.all(np.isfinite(df)) and np.all(np.isfinite(dg))
    _rows_past_the_lengths_are_zero(case, df, dg)
    assert ck.same_bits((nll, df, dg), _default_run((shape, 'random'))[:3])


def test_status_names_the_first_bad_utterance():
    """utterances 1 (a label = C-1) and 3 (enc_len = T + 1) are bad: status 2, their nll 0 and their rows zero; the
    good ones are what they are in a clean batch, bit for bit.  Then the other three causes, one at a time."""
    clean = tc.make_case(4, 20, 9, 5, 'random', 17)
    clean.label_len[:] = [5, 3, 2, 5]
    f, g, enc_len, labels, label_len = clean
    ref = ck.run(clean)
    assert ref[3] == 0
    labels2, enc2 = labels.copy(), enc_len.copy()
    labels2[1, 1] = 8
    enc2[3] = 21
    nll, df, dg, status = ck.run(tc.Case(f, g, enc2, labels2, label_len, {}))
    assert status == 2
    for b in (1, 3):
        assert nll[b] == 0 and np.all(df[b] == 0) and np.all(dg[b] == 0)
    for b in (0, 2):
        assert ck.same_bits((nll[b], df[b], dg[b]), (ref[0][b], ref[1][b], ref[2][b]))
    for b, change in ((2, ('enc', 0)), (3, ('len', 6)), (0, ('len', -1)), (1, ('lab', -1))):
        labels3, enc3, len3 = labels.copy(), enc_len.copy(), label_len.copy()
        if change[0] == 'enc':
            enc3[b] = change[1]
        elif change[0] == 'len':
            len3[b] = change[1]
        else:
            labels3[b, 0] = change[1]
        nll, df, dg, status = ck.run(tc.Case(f, g, enc3, labels3, len3, {}))
        assert status == 1 + b and nll[b] == 0 and np.all(df[b] == 0) and np.all(dg[b] == 0), (b, change)
        assert np.all(nll[[i for i in range(4) if i != b]] > 0)
    # a bad label past label_len is not read
    labels4 = labels.copy()
    labels4[2, 4] = -7
    assert ck.run(tc.Case(f, g, enc_len, labels4, label_len, {}))[3] == 0


def test_host_errors_return_before_any_launch():
    case = ck.case_of(((3, 12, 65, 6), 'random'))
    for kw, code in ((dict(T=0), -1), (dict(C=1), -1), (dict(nll=None), -1), (dict(ldl=5), -1), (dict(ws_less=1), -3)):
        rc, nll, df, dg, status, msg = _raw_call(case, 3.5, **kw)
        assert rc == code and msg, (kw, rc, msg)
        assert status == 77 and np.all(nll == 3.5) and np.all(df == 3.5) and np.all(dg == 3.5), kw
    from nabu_amd import _hip, ops
    import torch
    z = torch.zeros((2, 3, 4), device='cuda')
    i = torch.ones(2, dtype=torch.int32, device='cuda')
    with pytest.raises(_hip.NabuHipError):
        ops.transducer_loss_grad(z, torch.zeros((2, 2, 5), device='cuda'), i, i.view(2, 1), i, 1.0)


def _greedy_inputs(C, B=5, T=6, S=4):
    """f [B,T,C], the prediction logits gtab [B,S+1,C] after 0 .. S labels, enc_len — all on the quarter grid.  Noise in
    [-0.75, 0.75] with 3.25 on the blank of f: no label wins by chance (at most 1.5 against at least 1.75).  A planted
    emission of k at frame t puts 6, 5, .. on f[b,t,k] in the order wanted, and -8 on the labels that frame has already
    given in the prediction logits of the histories that follow, so the frame moves on."""
    blank = C - 1
    rng = np.random.default_rng(C)
    f = rng.integers(-3, 4, (B, T, C)) / 4.0
    gtab = rng.integers(-3, 4, (B, S + 1, C)) / 4.0
    f[:, :, blank] += 3.25
    plan = {0: [(3, [2])], 3: [(0, [1])], 4: [(1, [0, 3]), (2, [C - 3])]}        # row -> [(frame, labels in order)]
    f[0, 0, :], gtab[0, 0, :] = 0, 0
    f[0, 0, [1, blank]] = 4.0                                # row 0: label 1 ties with the blank
    gtab[0, 1, 1] = -8.0
    f[1, 0, :], gtab[1, 0, :] = 0, 0
    f[1, 0, 2], gtab[1, 0, 3] = 4.0, 4.0                     # row 1: labels 2 and 3 tie, 4 + 1 = 1 + 4
    f[1, 0, 3], gtab[1, 0, 2] = 1.0, 1.0
    f[1, 0, blank], gtab[1, 1, 2] = 3.25, -8.0
    f[2, :, 0] += 8.0                                        # row 2 emits label 0 until it holds S labels
    for b, frames in plan.items():
        n = 1 if b == 0 else 0                               # labels the row holds before the frame
        for t, ks in frames:
            for i, k in enumerate(ks):
                f[b, t, k] = 6.0 - i
                n += 1
                gtab[b, n, ks[:i + 1]] = -8.0
    return f, gtab, np.array([T, T - 1, T, 1, T - 2], np.int32), blank


@pytest.mark.parametrize('C', [5, 70])
def test_greedy_step(C):
    """2 T lock-step iterations on quarter-grid logits (every sum exact in float32): ids, out_len and t_pos equal the
    reference's.  Planted: row 0 an exact tie between label 1 and the blank (label 1 wins), row 1 between labels 2 and
    3 (2 wins), row 2 prefers labels throughout and reaches S, row 3 has enc_len = 1.  The state starts as garbage:
    step 0 sets it up."""
    import torch
    from nabu_amd import ops
    B, T, S = 5, 6, 4
    f, gtab, enc_len, blank = _greedy_inputs(C)
    r_ids, r_len, r_pos, r_score, margins, _ = tr.greedy_search(f, enc_len, S, lambda b, ids: gtab[b, len(ids)], 2 * T)
    assert margins[0][0] == 0 and margins[1][0] == 0 and r_ids[0, 0] == 1 and r_ids[1, 0] == 2      # the ties are there
    assert r_len[2] == S and r_pos[2] == 0 and r_pos[3] == 1 and np.all(r_pos[[0, 1, 4]] == enc_len[[0, 1, 4]])
    assert r_ids[0].tolist() == [1, 2, -1, -1] and r_ids[4].tolist() == [0, 3, C - 3, -1] and r_ids[3, 0] == 1

    fd = torch.as_tensor(f, dtype=torch.float32).cuda()
    gd = torch.as_tensor(gtab, dtype=torch.float32).cuda()
    el = torch.as_tensor(enc_len).cuda()
    t_pos, out_len, emit, last_id = (torch.full((B,), 12345, dtype=torch.int32, device='cuda') for _ in range(4))
    ids = torch.full((B, S), 999, dtype=torch.int32, device='cuda')
    score = torch.full((B,), float('nan'), device='cuda')
    rows = torch.arange(B, device='cuda')
    emits = []
    for step in range(2 * T):
        g_row = gd[rows, out_len.long()] if step else gd[:, 0]
        ops.transducer_greedy_step(step, fd, g_row.contiguous(), el, t_pos, out_len, ids, emit, last_id, score)
        emits.append(emit.cpu().numpy().copy())
    assert np.array_equal(ids.cpu().numpy(), r_ids) and np.array_equal(out_len.cpu().numpy(), r_len)
    assert np.array_equal(t_pos.cpu().numpy(), r_pos)
    assert np.array_equal(np.sum(emits, axis=0), r_len) and set(np.unique(emits)) <= {0, 1} and not emits[-1].any()
    want_last = [r_ids[b, r_len[b] - 1] if r_len[b] else blank for b in range(B)]
    assert last_id.cpu().numpy().tolist() == want_last
    assert np.allclose(score.cpu().numpy(), r_score, rtol=1e-5, atol=1e-5)
