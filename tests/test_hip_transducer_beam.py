"""nabu_transducer_beam_step (csrc/transducer_beam.hip) against the float64 restatement of tests/transducer_beam_ref.py:
step by step on the inputs of tests/transducer_beam_cases.py, a planted tie, the exact posteriors of an unpruned search
against the loss kernel, a beam of one against the greedy kernel, determinism and the host-side errors.

The prediction logits of every iteration come from a table keyed by the labels the device holds in each slot, read
back; the rows of empty slots are NaN, and so is f where no frame is."""
import itertools

import numpy as np
import pytest

from tests import transducer_beam_cases as bc
from tests import transducer_beam_ref as br
from tests import transducer_ref as tr
from tests.test_hip_transducer import _greedy_inputs

pytestmark = pytest.mark.gpu
KEYS = ('ids', 'out_len', 'score', 'parent', 'emit', 'last_id', 'fin_ids', 'fin_len', 'fin_score')
_ref = {}


def _reference(C, W):
    """the restatement's runs with and without the merge on beam_inputs(C): computed once, never changed"""
    if (C, W) not in _ref:
        f, enc_len, g_fn = bc.beam_inputs(C)
        _ref[C, W] = (f, enc_len, g_fn, br.beam_search(f, enc_len, bc.S, W, g_fn),
                      br.beam_search(f, enc_len, bc.S, W, g_fn, merge=False))
    return _ref[C, W]


def _garbage_state(B, W, S):
    import torch
    from nabu_amd import ops
    st = ops.transducer_beam_state(B, W, S, 'cuda')
    for k in KEYS:
        t = getattr(st, k)
        t.fill_(float('nan') if t.dtype == torch.float32 else 12345)
    st.ws.fill_(0xAB)
    return st


def _snapshot(st):
    return {k: getattr(st, k).cpu().numpy().copy() for k in KEYS}


def _search(f, enc_len, g_fn, S, W, iters, each=None):
    """`iters` iterations on the device from a garbage state; each(i, snapshot) after every one.  Returns the last
    snapshot"""
    import torch
    from nabu_amd import ops
    B, T, C = f.shape
    fd = torch.as_tensor(f, dtype=torch.float32).cuda()
    el = torch.as_tensor(np.asarray(enc_len, np.int32)).cuda()
    st = _garbage_state(B, W, S)
    snap = None
    for i in range(iters):
        g = np.full((B, W, C), np.nan, np.float32)
        for b in range(B):
            if i == 0:
                if min(max(int(enc_len[b]), 0), T) > 0:
                    g[b, 0] = g_fn(b, ())
                continue
            for w in range(W):
                n = snap['out_len'][b, w]
                if n >= 0:
                    g[b, w] = g_fn(b, tuple(int(k) for k in snap['ids'][b, w, :n]))
        ops.transducer_beam_step(i, fd, torch.as_tensor(g).cuda(), el, st)
        snap = _snapshot(st)
        if each:
            each(i, snap)
    return snap


def _same_beam(i, got, want):
    for k in ('ids', 'out_len', 'parent', 'emit', 'last_id', 'fin_ids', 'fin_len'):
        assert np.array_equal(got[k], want[k]), (i, k, got[k].tolist(), want[k].tolist())
    for sc, ln in (('score', 'out_len'), ('fin_score', 'fin_len')):
        live = want[ln] >= 0
        assert np.allclose(got[sc][live], want[sc][live], rtol=1e-5, atol=1e-5), (i, sc, got[sc], want[sc])
        assert np.all(np.isneginf(got[sc][~live])), (i, sc, got[sc])


@pytest.mark.parametrize('W', [1, 2, 4, 8])
@pytest.mark.parametrize('C', [3, 5, 70])
def test_step_by_step_against_the_trace(C, W):
    f, enc_len, g_fn, res, plain = _reference(C, W)
    bad = bc.conditions(res, plain, W)                   # the CONDITIONS, on the restatement alone
    print('C %d W %d: margin %.3e, merges %s, shrinks %s, capped %s, finals %s' %
          (C, W, res['margin'], res['merges'], res['shrinks'], res['capped'], [len(x) for x in res['finals']]))
    assert bad == [], bad
    last = _search(f, enc_len, g_fn, bc.S, W, bc.T + bc.S, lambda i, snap: _same_beam(i, snap, res['trace'][i]))
    assert np.all(last['out_len'] == -1)                 # every utterance is done
    ids, lens, scores = br.best(res['finals'], bc.S)
    assert np.array_equal(last['fin_ids'][:, 0], ids) and np.array_equal(last['fin_len'][:, 0], lens)


@pytest.mark.parametrize('C,W', [(3, 2), (3, 4), (5, 4), (5, 8), (70, 8)])
def test_planted_tie(C, W):
    """every logit of the first iteration is equal: the survivors are the labels 0 .. W-1 in that order, and the
    blank, with the largest flat index, survives only when W >= C"""
    T, S = 3, 2
    f = np.zeros((2, T, C))
    f[:, 1:] = np.random.default_rng(C).integers(-3, 4, (2, T - 1, C)) / 4.0
    enc_len = [T, 1]                                     # utterance 1: that blank completes () instead
    first = []
    _search(f, enc_len, lambda b, y: np.zeros(C), S, W, 1, lambda i, snap: first.append(snap))
    got = first[0]
    n = min(W, C - 1)
    for b in range(2):
        assert got['ids'][b, :n, 0].tolist() == list(range(n)) and got['last_id'][b, :n].tolist() == list(range(n))
        assert got['out_len'][b, :n].tolist() == [1] * n and got['emit'][b, :n].tolist() == [1] * n
    if W >= C:
        assert got['out_len'][0, n] == 0 and got['emit'][0, n] == 0 and got['parent'][0, n] == 0
        assert got['out_len'][1, n] == -1 and got['fin_len'][1].tolist() == [0] + [-1] * (W - 1)
        assert np.all(got['out_len'][0, n + 1:] == -1)
    else:
        assert np.all(got['out_len'][:, n:] == -1) and np.all(got['fin_len'] == -1)
    want = br.beam_search(f, enc_len, S, W, lambda b, y: np.zeros(C), iters=1)['trace'][0]
    _same_beam(0, got, want)


def test_exact_posteriors_against_the_loss_kernel():
    """C 3, T 4, S 2, W 8: nothing is pruned, so every final's score is log P(y | x) — what the loss kernel returns as
    -nll on the same f with g stacked from the same table.  Both within 1e-5 of the float64 restatement, and within
    twice that of each other"""
    import torch
    from nabu_amd import ops
    C, T, S, W = 3, 4, 2, 8
    rng = np.random.default_rng(11)
    f = rng.standard_normal((1, T, C)).astype(np.float32).astype(np.float64)
    tab = {y: rng.standard_normal(C).astype(np.float32).astype(np.float64)
           for n in range(S + 1) for y in itertools.product(range(C - 1), repeat=n)}
    g_fn = lambda b, y: tab[tuple(y)]                    # noqa: E731
    want = dict(br.beam_search(f, [T], S, W, g_fn)['finals'][0])
    assert len(want) == 7
    last = _search(f, [T], g_fn, S, W, T + S)
    got = {tuple(int(k) for k in last['fin_ids'][0, j, :last['fin_len'][0, j]]): float(last['fin_score'][0, j])
           for j in range(W) if last['fin_len'][0, j] >= 0}
    assert sorted(got) == sorted(want)
    assert list(last['fin_score'][0, :7]) == sorted(last['fin_score'][0, :7], reverse=True) and last['fin_len'][0, 7] == -1
    seqs = sorted(want)
    g = np.zeros((len(seqs), S + 1, C), np.float32)
    labels = np.zeros((len(seqs), S), np.int32)
    for r, y in enumerate(seqs):
        labels[r, :len(y)] = y
        for u in range(len(y) + 1):
            g[r, u] = tab[y[:u]]
    fd = torch.as_tensor(np.repeat(f, len(seqs), 0), dtype=torch.float32).cuda().contiguous()
    nll = ops.transducer_loss_grad(fd, torch.as_tensor(g).cuda(), torch.full((len(seqs),), T, dtype=torch.int32, device='cuda'),
                                   torch.as_tensor(labels).cuda(),
                                   torch.as_tensor(np.array([len(y) for y in seqs], np.int32)).cuda(), 1.0)[0].cpu().numpy()
    for r, y in enumerate(seqs):
        exact = -tr.brute_force_nll(f[0], np.stack([tab[y[:u]] for u in range(len(y) + 1)]), list(y))[0]
        print(y, 'beam %.7f loss %.7f float64 %.7f enumeration %.7f' % (got[y], -nll[r], want[y], exact))
        assert abs(want[y] - exact) < 1e-12
        assert abs(got[y] - want[y]) <= 1e-5 and abs(-nll[r] - want[y]) <= 1e-5 and abs(got[y] + nll[r]) <= 2e-5


@pytest.mark.parametrize('C', [5, 70])
def test_beam_of_one_against_the_greedy_kernel(C):
    import torch
    from nabu_amd import ops
    B, T, S = 5, 6, 4
    f, gtab, enc_len, blank = _greedy_inputs(C)
    fd = torch.as_tensor(f, dtype=torch.float32).cuda()
    gd = torch.as_tensor(gtab, dtype=torch.float32).cuda()
    el = torch.as_tensor(enc_len).cuda()
    t_pos, out_len, emit, last_id = (torch.full((B,), 12345, dtype=torch.int32, device='cuda') for _ in range(4))
    ids = torch.full((B, S), 999, dtype=torch.int32, device='cuda')
    score = torch.full((B,), float('nan'), device='cuda')
    rows = torch.arange(B, device='cuda')
    for step in range(T + S):
        g_row = gd[rows, out_len.long()] if step else gd[:, 0]
        ops.transducer_greedy_step(step, fd, g_row.contiguous(), el, t_pos, out_len, ids, emit, last_id, score)
    last = _search(f, enc_len, lambda b, y: gtab[b, len(y)], S, 1, T + S)
    assert np.array_equal(last['fin_ids'][:, 0], ids.cpu().numpy())
    assert np.array_equal(last['fin_len'][:, 0], out_len.cpu().numpy())
    out = t_pos.cpu().numpy() >= np.minimum(enc_len, T)
    assert out.sum() >= 3 and not out.all()
    assert np.allclose(last['fin_score'][out, 0], score.cpu().numpy()[out], rtol=1e-5, atol=1e-5)


def test_two_searches_give_the_same_bits():
    f, enc_len, g_fn, _, _ = _reference(70, 8)
    runs = []
    for _ in range(2):
        snaps = []
        _search(f, enc_len, g_fn, bc.S, 8, bc.T + bc.S, lambda i, snap: snaps.append(snap))
        runs.append(snaps)
    for a, b in zip(*runs):
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k


def test_host_errors_return_before_any_launch():
    import torch
    from nabu_amd import _hip
    B, T, C, S, W = 2, 3, 4, 2, 3
    L = _hip.lib()
    fd = torch.zeros((B, T, C), device='cuda')
    gd = torch.zeros((B, W, C), device='cuda')
    el = torch.full((B,), T, dtype=torch.int32, device='cuda')
    st = _garbage_state(B, W, S)
    before = _snapshot(st)
    wsb = L.nabu_transducer_beam_ws_bytes(B, W, C, S)
    assert wsb >= B * W * S * 4 and L.nabu_transducer_beam_ws_bytes(0, W, C, S) == 0
    names = ('f', 'g_rows', 'enc_len') + KEYS + ('ws',)

    def call(**over):
        a = dict(B=B, T=T, C=C, S=S, W=W, step=0, ws_bytes=wsb, f=_hip.ptr(fd), g_rows=_hip.ptr(gd), enc_len=_hip.ptr(el),
                 ws=_hip.ptr(st.ws), **{k: _hip.ptr(getattr(st, k)) for k in KEYS})
        a.update(over)
        rc = L.nabu_transducer_beam_step(a['B'], a['T'], a['C'], a['S'], a['W'], a['step'], *[a[n] for n in names[:-1]],
                                         a['ws'], a['ws_bytes'], _hip.stream())
        torch.cuda.synchronize()
        return rc, L.nabu_last_error().decode()
    cases = [(dict(W=0), -1, 'W='), (dict(W=33), -1, 'W='), (dict(B=0), -1, 'B='), (dict(B=65536), -1, 'B='),
             (dict(S=0), -1, 'S='), (dict(C=1), -1, 'C='), (dict(step=-1), -1, 'step='), (dict(T=0), -1, 'T='),
             (dict(ws_bytes=wsb - 1), -3, 'ws_bytes')]
    cases += [({n: None}, -1, n) for n in names]
    for over, code, word in cases:
        rc, msg = call(**over)
        assert rc == code and word in msg, (over, rc, msg)
        after = _snapshot(st)
        assert all(after[k].tobytes() == before[k].tobytes() for k in KEYS), over
    # 4 W (C + S) bytes of LDS, more than a CU has: refused before the launch (ws_bytes only has to pass its own check)
    rc, msg = call(W=32, C=4000, ws_bytes=1 << 20)
    assert rc == -2 and 'LDS' in msg, (rc, msg)
    rc, _ = call()
    assert rc == 0
