"""Scheduled-sampling draws of every HIP sampling kernel against the host Philox
reference (oracle/philox.py): nabu_sample_ids directly, the step chain's
sample_step kernel and its GEMM + sample_ids fallback, the persistent decoder's
sample_row, and the Python bookkeeping that turns the global RNG into the
sampling offset.

Rule of every comparison: the Bernoulli selections match the host exactly; the
drawn ids match the host's float64 inverse CDF exactly, except in rows whose
u * total lies within 1e-5 * total of a class boundary of the CDF.  Such a row
may land on any class the band touches (and nothing else), and such rows are
few (near_boundary_limit)."""
import os

import numpy as np
import pytest
import torch

from oracle import nabu_oracle as O
from oracle import philox as P
from nabu_amd import recipes

pytestmark = pytest.mark.gpu

PRE = 'Speller/decoder/'
SCOPES = {'vanilla': 'bahdanau_attention', 'location_aware': 'location_aware_attention',
          'windowed': 'windowed_attention'}


def near_boundary_limit(C, draws):
    """Largest allowed number of draws within 1e-5 * total of a CDF boundary.  Each of the C - 1 boundaries
    claims a band 2e-5 wide of the unit interval, so by chance up to 2e-5 (C - 1) of the draws fall near one:
    0.5 % of the draws, or three times that expectation where it is larger (C > 84), plus two rows for the
    chance of a few hundred draws."""
    return max(0.005, 6e-5 * (C - 1)) * draws + 2


class DrawStats(object):
    """draws compared with the host, strict mismatches, near-boundary rows (and out-of-band ones among them)"""

    def __init__(self, C):
        self.C, self.draws, self.rows, self.mismatched, self.near, self.near_bad = C, 0, 0, 0, 0, 0

    def add(self, got, logits, prob, seed, offset, teacher, rows=None):
        """got [B] ids the kernel chose for logits [B, C] at (seed, offset); rows: mask of the rows to compare"""
        ids, sel, margin, bounds = P.reference_draw(logits, prob, seed, offset, teacher)
        rows = np.ones(len(got), bool) if rows is None else rows
        got = np.asarray(got, np.int64)
        near = sel & (margin <= 1e-5)
        strict = rows & ~near
        self.rows += int(rows.sum())
        self.draws += int((rows & sel).sum())
        self.mismatched += int((got[strict] != ids[strict]).sum())
        nr = rows & near
        self.near += int(nr.sum())
        self.near_bad += int(((got[nr] < bounds[nr, 0]) | (got[nr] > bounds[nr, 1])).sum())
        return sel

    def check(self, what):
        msg = '%s C=%d: %d draws (%d rows), %d mismatched (%.4f), %d near a boundary (%d outside its band)' % (
            what, self.C, self.draws, self.rows, self.mismatched, self.mismatched / max(self.draws, 1), self.near,
            self.near_bad)
        print(msg)
        assert self.draws > 0, msg
        assert self.mismatched == 0 and self.near_bad == 0, msg
        assert self.near <= near_boundary_limit(self.C, self.draws), msg


# ----------------------------------------------------------------------------------------------- nabu_sample_ids


def _logits(kind, B, C, rng):
    if kind == 'dominant':            # one class per row far above the rest
        lg = rng.normal(size=(B, C))
        lg[np.arange(B), rng.integers(0, C, B)] += 12.0
    elif kind == 'uniform':           # near-uniform: C - 1 boundaries spread over the whole unit interval
        lg = 1e-3 * rng.normal(size=(B, C))
    else:
        lg = 2.0 * rng.normal(size=(B, C))
    return lg.astype(np.float32)


@pytest.mark.parametrize('C', [2, 3, 40, 47, 48, 64, 65, 256, 1000])
def test_sample_ids_draws_match_the_host(C):
    """B = 300 rows (two workgroups, rows above 255), prob 0 / 0.3 / 1, dominant, near-uniform and spread logits;
    teacher ids out of the class range, so the Bernoulli selection is visible in every row"""
    from nabu_amd import ops
    B = 300
    rng = np.random.default_rng(1000 + C)
    st = DrawStats(C)
    teacher = (C + np.arange(B)).astype(np.int32)
    td = torch.tensor(teacher, device='cuda')
    for kind in ('dominant', 'uniform', 'spread'):
        lg = _logits(kind, B, C, rng)
        lgd = torch.tensor(lg, device='cuda')
        for prob, seed, offset in ((0.0, 7, 3), (0.3, 12345, (5 << 32) + 1000003 * 9 + 4), (1.0, (1 << 40) + 3, 77)):
            got = ops.sample_ids(lgd, prob, seed, offset, td).cpu().numpy()
            sel = st.add(got, lg, prob, seed, offset, teacher)
            np.testing.assert_array_equal(got >= C, ~sel)                  # the Bernoulli, bit for bit
            np.testing.assert_array_equal(got[~sel], teacher[~sel])
            if prob == 0.3:
                assert 0.15 < sel.mean() < 0.45
    st.check('sample_ids')


# ------------------------------------------------------------------------------------------------ decoder runs


def _data(rng, B, Te, E, C, tmin, tmax):
    enc_len = rng.integers(Te // 2, Te + 1, B).astype(np.int32)
    enc_len[0] = Te
    tlen = rng.integers(tmin, tmax + 1, B).astype(np.int32)
    tlen[1] = tmax
    enc = rng.normal(size=(B, Te, E)).astype(np.float32)
    enc *= (np.arange(Te)[None, :, None] < enc_len[:, None, None])
    tg = rng.integers(0, C - 1, (B, tmax)).astype(np.int32)
    for b in range(B):
        tg[b, tlen[b] - 1] = C - 1
        tg[b, tlen[b]:] = 0
    return enc, enc_len, tg, tlen


class Decoder(object):
    """a Speller built from the cfg3 recipe + over, with its own variable store; call() runs it once on the GPU"""

    def __init__(self, over, C):
        from nabu_amd import variables as vs
        from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory
        mc, _, _ = recipes.load_recipe('cfg3_las_vanilla', **over)
        self.dec = ed_decoder_factory.factory('speller')(mc, {'text': C}, None)
        self.store = vs.VariableStore(seed=3)
        self.C, self.over = C, over

    def call(self, enc, enc_len, tg, tlen, backward=False):
        """logits [B, L, C], the decoder inputs used [L, B], the paths taken, the sampling (seed, offset of step 0)
        as dynamic_decode derives them from the global RNG, and the loss (after its backward, if asked)"""
        from nabu_amd import variables as vs
        from nabu_amd.autodiff import Tape, SeqLen
        from nabu_amd.neuralnetworks.components import ops as nops
        from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
        from nabu_amd.neuralnetworks.trainers import loss_functions
        dev = torch.device('cuda')
        L = int(tlen.max())
        nl = int(self.over['decoder.num_layers'])
        keep = float(self.over.get('decoder.dropout', 1.0))
        rs = nops.global_rng()
        seed, off = rs.seed, rs.offset
        if keep < 1:
            off += 1 + L * nl            # the dropout stream: one draw, then one mask per (step, layer)
        off += 1
        tgd = torch.tensor(tg, device=dev)
        with vs.as_default(self.store), Tape() as tape:
            logits, lsl, _ = self.dec({'features': torch.tensor(enc, device=dev)}, {'features': SeqLen(enc_len, dev)},
                                      {'text': tgd}, {'text': SeqLen(tlen, dev)}, True)
            loss = loss_functions.average_cross_entropy({'text': tgd}, logits, lsl, {'text': SeqLen(tlen, dev)})
        assert (rs.seed, rs.offset) == (seed, off + L)      # the sampling stream reserves one offset per step
        used = rnn_decoder.decoder_inputs().cpu().numpy().copy()
        paths = rnn_decoder.dynamic_decode.last_paths
        if backward:
            tape.backward(loss)
        return logits['text'].cpu().numpy(), used, paths, (seed, off * 1000003), loss


def teacher_inputs(tg, tlen, C):
    """[L, B]: SOS, then the targets shifted by one"""
    L = int(tlen.max())
    return np.concatenate([np.full((1, len(tlen)), C - 1), tg[:, :L - 1].T], 0).astype(np.int64)


def check_decoder_draws(st, logits, used, tg, tlen, prob, seed, offset0):
    """the input of step t + 1 of every utterance still running there against the host draw from the logits the
    decoder returned for step t (Philox offset offset0 + t, counter row = the global row)"""
    C = st.C
    teacher = teacher_inputs(tg, tlen, C)
    assert np.all(used[0] == C - 1)
    for t in range(int(tlen.max()) - 1):
        rows = t + 1 < tlen
        sel = st.add(used[t + 1], logits[:, t].astype(np.float64), prob, seed, offset0 + t, teacher[t + 1], rows)
        # rows the Bernoulli passes over keep the teacher's input exactly
        np.testing.assert_array_equal(used[t + 1][rows & ~sel], teacher[t + 1][rows & ~sel])


class chain_only(object):
    """NABU_SPELLER_PERSIST=0 and _BWD=0: the step chain, whatever the geometry"""

    def __enter__(self):
        os.environ['NABU_SPELLER_PERSIST'] = os.environ['NABU_SPELLER_PERSIST_BWD'] = '0'

    def __exit__(self, *a):
        del os.environ['NABU_SPELLER_PERSIST'], os.environ['NABU_SPELLER_PERSIST_BWD']


# C % 4 == 0, 4 <= C <= 256: sample_step (both sides of 256 / (C / 4) = 25, the largest C it takes);
# 47 and 257: the GEMM + sample_ids_rows fallback
CHAIN_CS = [8, 40, 44, 48, 52, 64, 100, 128, 252, 256, 47, 257]


@pytest.mark.parametrize('nl', [1, 2])
@pytest.mark.parametrize('C', CHAIN_CS)
def test_step_chain_draws_match_the_host(C, nl):
    """sample_prob 1: every row of every step is a draw.  32 utterances run as two sub-batches of 16 on two
    streams, so the second's rows enter the Philox counter at b0 = 16"""
    from nabu_amd.neuralnetworks.components import ops as nops
    rng = np.random.default_rng(C + 10 * nl)
    B, Te, E, U = 32, 21, 64, 64
    enc, enc_len, tg, tlen = _data(rng, B, Te, E, C, 16, 26)
    over = {'decoder.num_layers': nl, 'decoder.num_units': U, 'decoder.attention': 'vanilla',
            'decoder.sample_prob': 1.0}
    nops.set_seed(2 + C)
    with chain_only():
        logits, used, paths, (seed, off), _ = Decoder(over, C).call(enc, enc_len, tg, tlen)
    assert paths == (0, 0)
    st = DrawStats(C)
    check_decoder_draws(st, logits, used, tg, tlen, 1.0, seed, off)
    st.check('step chain (%d layer%s)' % (nl, 's' if nl > 1 else ''))


@pytest.mark.parametrize('attention', ['vanilla', 'location_aware'])
@pytest.mark.parametrize('C', [48, 64, 47, 63, 68])
def test_persistent_decoder_draws_match_the_host(attention, C):
    """sample_row of the persistent decoder: C % 4 == 0 (48, 64) takes the class-quad branch, 47 and 63 the
    lane-per-class one; C = 68 is past what the persistent kernel samples and runs as the step chain"""
    from nabu_amd import ops as hip
    from nabu_amd.neuralnetworks.components import ops as nops
    rng = np.random.default_rng(300 + C)
    B, Te, E, U = 32, 33, 64, 64
    enc, enc_len, tg, tlen = _data(rng, B, Te, E, C, 20, 30)
    over = {'decoder.num_layers': 1, 'decoder.num_units': U, 'decoder.attention': attention,
            'decoder.sample_prob': 0.5}
    if attention == 'location_aware':
        over.update({'decoder.numfilt': 3, 'decoder.filtersize': 7})
    nops.set_seed(40 + C)
    logits, used, paths, (seed, off), _ = Decoder(over, C).call(enc, enc_len, tg, tlen)
    hip.check_persist_status()
    assert paths[0] == (1 if C <= 64 else 0), paths
    st = DrawStats(C)
    check_decoder_draws(st, logits, used, tg, tlen, 0.5, seed, off)
    st.check(('persistent decoder (%s)' if C <= 64 else 'fallback of the persistent decoder (%s)') % attention)


def _speller_params(st, nl, attention):
    sc = SCOPES[attention]
    p = dict(memory_kernel=st[PRE + 'memory_layer/kernel'], query_kernel=st[PRE + sc + '/query_layer/kernel'],
             attention_v=st[PRE + sc + '/attention_v'], out_kernel=st[PRE + 'dense/kernel'],
             out_bias=st[PRE + 'dense/bias'], lstm=[])
    for n in range(nl):
        q = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        p['lstm'].append(dict(kernel=st[q + 'kernel'], bias=st[q + 'bias']))
    f64 = lambda v: [{k: a.astype(np.float64) for k, a in d.items()} for d in v] if isinstance(v, list) \
        else v.astype(np.float64)
    return {k: f64(v) for k, v in p.items()}


def test_las_gp_geometry_draws_and_oracle():
    """The reference's LAS/GP decoder (47 labels + 1 = 48 classes, 2 layers of 128 units, windowed attention 10 / 15
    frames) at the default sample_prob 0.1: draws against the host; logits, loss and every gradient against the
    oracle run on the inputs the decoder actually used"""
    rng = np.random.default_rng(47)
    B, Te, E, C, U, nl = 32, 50, 256, 48, 128, 2
    enc, enc_len, tg, tlen = _data(rng, B, Te, E, C, 10, 24)
    enc *= 0.3
    over = {'decoder.num_layers': nl, 'decoder.num_units': U, 'decoder.attention': 'windowed',
            'decoder.left_window_width': 10, 'decoder.right_window_width': 15, 'decoder.sample_prob': 0.1}
    from nabu_amd.neuralnetworks.components import ops as nops
    nops.set_seed(11)
    d = Decoder(over, C)
    logits, used, paths, (seed, off), loss = d.call(enc, enc_len, tg, tlen, backward=True)
    assert paths == (0, 0)                           # two layers: never the persistent kernel
    st = DrawStats(C)
    check_decoder_draws(st, logits, used, tg, tlen, 0.1, seed, off)
    st.check('LAS/GP geometry')
    teacher = teacher_inputs(tg, tlen, C)
    live = np.arange(int(tlen.max()))[:, None] < tlen[None, :] - 1
    assert (used[1:] != teacher[1:])[live[:-1]].any()               # some inputs really were drawn
    # the reference is not circular: the logits themselves against the oracle fed the inputs used
    p = _speller_params(d.store.state_dict(), nl, 'windowed')
    rl, rll, cache = O.speller_fwd(enc.astype(np.float64), enc_len, tg, tlen, p, 'windowed', dec_inputs=used.T,
                                   window=(10, 15))
    assert np.abs(logits - rl).max() < 2e-5
    rloss, dlg = O.average_cross_entropy(rl, tg, rll, tlen)
    assert abs(float(loss.item()) - rloss) / rloss < 1e-5
    _, rg = O.speller_bwd(dlg, cache)
    rel = lambda a, b_: np.abs(a - b_).max() / (np.abs(b_).max() + 1e-12)
    sc = SCOPES['windowed']
    names = {'memory_kernel': PRE + 'memory_layer/kernel', 'query_kernel': PRE + sc + '/query_layer/kernel',
             'attention_v': PRE + sc + '/attention_v', 'out_kernel': PRE + 'dense/kernel', 'out_bias': PRE + 'dense/bias'}
    for k, name in names.items():
        g = d.store.vars[name].grad.cpu().numpy().astype(np.float64).reshape(rg[k].shape)
        assert rel(g, rg[k]) < 2e-4, k
    for n in range(nl):
        q = PRE + 'attention_wrapper/multi_rnn_cell/cell_%d/lstm_cell/' % n
        assert rel(d.store.vars[q + 'kernel'].grad.cpu().numpy(), rg['lstm'][n]['kernel']) < 2e-4, n
        assert rel(d.store.vars[q + 'bias'].grad.cpu().numpy(), rg['lstm'][n]['bias']) < 2e-4, n


@pytest.mark.parametrize('dropout', [1.0, 0.8])
def test_consecutive_calls_advance_the_sampling_offset(dropout):
    """two calls of one decoder: the second draws at the offset the first left the global RNG at (after the
    dropout stream's reservation, with output dropout) -- the host's draws there, and not the first call's"""
    from nabu_amd.neuralnetworks.components import ops as nops
    rng = np.random.default_rng(5)
    B, Te, E, U, C = 32, 21, 64, 64, 40
    enc, enc_len, tg, tlen = _data(rng, B, Te, E, C, 8, 14)
    over = {'decoder.num_layers': 1, 'decoder.num_units': U, 'decoder.attention': 'vanilla',
            'decoder.dropout': dropout, 'decoder.sample_prob': 0.5}
    nops.set_seed(9)
    d = Decoder(over, C)
    first = d.call(enc, enc_len, tg, tlen)
    second = d.call(enc, enc_len, tg, tlen)
    L = int(tlen.max())
    step = (1 + L if dropout < 1 else 0) + 1 + L                    # what one call takes from the global RNG
    assert first[3][0] == second[3][0] == 9
    assert (first[3][1], second[3][1]) == ((step - L) * 1000003, (2 * step - L) * 1000003)
    for logits, used, _, (seed, off), _ in (first, second):
        st = DrawStats(C)
        check_decoder_draws(st, logits, used, tg, tlen, 0.5, seed, off)
        st.check('call at offset %d' % off)
    live = np.arange(1, L)[:, None] < tlen[None, :]
    assert not np.array_equal(first[1][1:][live], second[1][1:][live])
