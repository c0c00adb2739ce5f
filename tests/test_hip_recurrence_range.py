"""The persistent BLSTM recurrences at extreme operand magnitudes (LABNOTES section 23): saturated gates, batch rows
whose gradients differ by 2^192, all-zero rows, a W_h whose rows and columns span 2^14, x at the edges of the in-kernel
projection's single scale, and the sigmoid at the argument where exp(-x) leaves float32.

Every case runs on each persistent kernel family (lstm_persist_plan) at the smallest shape that selects it, against
the float64 oracle on operands rounded through float32, at the bounds of test_blstm_persistent_matches_oracle.  The
step-wise kernels are no reference here: when a check fails they are run on the same operands and their errors are
printed beside the persistent kernels', to show which path is off.
"""
import numpy as np
import pytest

from tests.test_hip_ops import _blstm_operands, _run_blstm, rel_err

pytestmark = pytest.mark.gpu

# (B, T, D, H, recurrent_precision): which kernels take the shape is lstm_persist_plan's decision
FAMILIES = {
    'mxh_xin': (8, 12, 8, 128, 'default'),      # fp16 planes, the input projection inside the kernel (D <= 64)
    'mxh_gemm': (9, 12, 72, 256, 'default'),    # fp16 planes, projection by a GEMM; two units, the second with one row
    'mxf': (40, 6, 16, 512, 'default'),         # 32 hidden units per workgroup (33 .. 64 rows at H = 512)
    'f32_shape': (8, 12, 8, 64, 'default'),     # exact fp32: H = 64 has no fp16-plane kernel
    'f32_asked': (8, 12, 8, 128, 'f32'),        # exact fp32 by the per-call switch
}
FAMILY_IDS = list(FAMILIES)
GATE_I, GATE_J, GATE_F, GATE_O = 0, 1, 2, 3     # column blocks of the kernel and the bias (i, j, f, o; j is the tanh gate)

SATURATING = (-88., -89., -104., -300., -690., 88., 89., 104., 300., 690.)


def ragged(B, T):
    """lens[0] = T, one row of length 1, the others in between"""
    pat = [T, 1, T - 1, max(2, T // 2), T - 2, 3, T, T // 3 + 1]
    return [min(T, pat[b % len(pat)]) for b in range(B)]


def saturating_bias(bias, H):
    """for each gate ten units of its own (40 distinct units) at the SATURATING values, in place; returns the units whose
    OUTPUT gate sits at <= -89.  |bias| <= 690 keeps the float64 oracle's own exp finite."""
    assert H >= 40 and bias.shape == (4 * H,)
    for g in range(4):
        for j, v in enumerate(SATURATING):
            bias[g * H + 10 * g + j] = v
    return [10 * GATE_O + j for j, v in enumerate(SATURATING) if v <= -89.]


def check(family, edit, per_row_dx=False, out_only=False, oracle_overflows=False):
    """one forward + backward call of the persistent kernels on the edited operands, against the oracle.  Returns
    (out, ref_out, dx, ref_dx, lens) for the case's own assertions.  oracle_overflows: the case drives the oracle's own
    exp beyond float64 (its sigmoid is then 1 / inf = 0, the limit); its results must be finite all the same."""
    from nabu_amd import ops
    B, T, D, H, rp = FAMILIES[family]
    lens = ragged(B, T)
    with np.errstate(over='ignore' if oracle_overflows else 'raise'):
        opr = _blstm_operands(B, T, D, H, lens, seed=B + H, edit=edit)
    x, p, dout, rout, rdx, rg = opr
    assert np.isfinite(rout).all() and np.isfinite(rdx).all() and all(np.isfinite(v).all() for v in rg.values())

    def errors(mode, rp):
        out, _, dx, _, g, _ = _run_blstm(B, T, D, H, lens, mode, recurrent_precision=rp, operands=opr)
        ops.check_persist_status()
        e = {'finite': bool(np.isfinite(out).all() and np.isfinite(dx).all() and all(np.isfinite(v).all() for v in g.values())),
             'out': np.abs(out - rout).max(),
             'past_len': max([np.abs(out[b, n:]).max() for b, n in enumerate(lens) if n < T] + [0.0]),
             'tiny': np.abs(out[np.abs(rout) < 1e-38]).max() if (np.abs(rout) < 1e-38).any() else 0.0}
        if per_row_dx:      # the backward pass is linear in dout and rows meet in the weight gradients only
            rows = [b for b in range(B) if np.abs(dout[b]).max() > 0]
            e['dx'] = max(rel_err(dx[b], rdx[b]) for b in rows)
            e['dx_zero_rows'] = max([np.abs(dx[b]).max() for b in range(B) if b not in rows] + [0.0])
        else:
            e['dx'] = rel_err(dx, rdx)
        for k in rg:
            e[k] = rel_err(g[k], rg[k])
        return {k: v if isinstance(v, bool) else float(v) for k, v in e.items()}, out, dx

    e, out, dx = errors(ops.LSTM_PERSISTENT, rp)
    print('%s persistent: %s' % (family, {k: v if isinstance(v, bool) else float('%.3g' % v) for k, v in e.items()}))
    ok = (e['finite'] and e['out'] < (2e-5 if H <= 128 else 2e-4) and e['past_len'] == 0 and e['tiny'] < 1e-30
          and (out_only or (e['dx'] < 3e-4 and all(e[k] < 3e-4 for k in rg) and e.get('dx_zero_rows', 0.0) < 1e-30)))
    if not ok:
        with np.errstate(all='ignore'):
            third = errors(ops.LSTM_STEPWISE, 'default')[0]
        raise AssertionError('%s: persistent %r\nstep-wise kernels on the same operands %r' % (family, e, third))
    return out, rout, dx, rdx, lens


@pytest.mark.parametrize('family', FAMILY_IDS)
def test_saturated_gates_through_the_bias(family):
    """(a) every gate at -88, -89, -104, -300, -690 and the same positive, on units of its own, both directions: finite,
    the bounds, and an output gate at <= -89 closes the unit (|out| < 1e-30 at every visited frame)"""
    H = FAMILIES[family][3]
    closed = []

    def edit(x, p, dout):
        closed[:] = saturating_bias(p['fw_bias'], H)
        saturating_bias(p['bw_bias'], H)
    out, rout, _, _, lens = check(family, edit)
    for u in closed:
        assert np.abs(out[:, :, [u, H + u]]).max() < 1e-30, u


@pytest.mark.parametrize('family', FAMILY_IDS)
def test_saturated_gates_through_the_weights(family):
    """(b) one sigmoid-gate column and one tanh-gate column of W_h times 2^6 (|w| ~ 13: pre-activations in the hundreds,
    of either sign, and a 2^6 step in the forward planes' per-column scale); where the input goes through a GEMM
    (D = 72) a column of W_x of each kind as well"""
    B, T, D, H, _ = FAMILIES[family]

    def edit(x, p, dout):
        for k, (uo, uj, uf) in (('fw_kernel', (5, 9, 20)), ('bw_kernel', (6, 10, 21))):
            p[k][D:, GATE_O * H + uo] *= 64.0
            p[k][D:, GATE_J * H + uj] *= 64.0
            p[k][D:, GATE_F * H + uf] *= 64.0
            if D > 64:
                p[k][:D, GATE_I * H + uo + 20] *= 64.0
                p[k][:D, GATE_J * H + uj + 20] *= 64.0
    check(family, edit)


@pytest.mark.parametrize('family', FAMILY_IDS)
def test_gradient_magnitude_per_batch_row(family):
    """(c) dout[b] times 2^k(b), k in -96 .. +96; one row all zero, one row non-zero at a single frame and unit.  dx is
    compared PER ROW (a dz scale shared among the rows of a unit would lose the small rows); the zero row's dx stays
    below 1e-30 (zeros travel the tagged ring as the smallest denormal); the weight gradients, dominated by the 2^96
    rows, show that nothing overflowed"""
    B, T, D, H, _ = FAMILIES[family]
    ks = (-96, -48, -16, 0, 16, 48, 96)

    def edit(x, p, dout):
        for b in range(B):
            dout[b] *= 2.0 ** ks[b % 7]
        dout[3] = 0
        one = dout[4, 0, H + 3]             # a unit of the backward direction: its frame 0 is the LAST step, every frame has a gradient
        dout[4] = 0
        dout[4, 0, H + 3] = one
    check(family, edit, per_row_dx=True)


@pytest.mark.parametrize('zero', [False, True], ids=['scaled', 'zero'])
@pytest.mark.parametrize('family', FAMILY_IDS)
def test_structured_recurrent_weights(family, zero):
    """(d) W_h with rows scaled by 2^-12 .. 2^1, columns by 2^-12 .. 2^2, an all-zero row and an all-zero column among the
    first workgroup's 16 units, a column of N(0, 0.02) with a single 8.0 — every per-column (forward) and per-row
    (W_h^T, backward) plane scale differs from its neighbour's; and W_h = 0: every scale takes the amax = 0 path"""
    B, T, D, H, _ = FAMILIES[family]

    def edit(x, p, dout):
        rng = np.random.default_rng(7)
        for k in ('fw_kernel', 'bw_kernel'):
            wh = p[k][D:]
            if zero:
                wh[:] = 0
                continue
            wh *= 2.0 ** (np.arange(H) % 14 - 12.0)[:, None]
            wh *= 2.0 ** (np.arange(4 * H) % 15 - 12.0)[None, :]
            wh[7, :] = 0
            wh[:, GATE_I * H + 4] = 0
            wh[:, GATE_O * H + 9] = rng.normal(0, 0.02, H)
            wh[17, GATE_O * H + 9] = 8.0
    check(family, edit)


@pytest.mark.parametrize('variant', ['zero', 'one_element', 'tiny', 'outlier'])
def test_x_at_the_edges_of_the_projection_scale(variant):
    """(e) the in-kernel projection scales all of x by ONE power of two (lstm_mxh_prepare_x): x = 0, x zero but one
    element, x 2^-60, and x N(0, 1) with one element of 2^12 (that frame's gates saturate)"""
    def edit(x, p, dout):
        if variant == 'zero':
            x[:] = 0
        elif variant == 'one_element':
            v = x[2, 1, 3]
            x[:] = 0
            x[2, 1, 3] = v
        elif variant == 'tiny':
            x *= 2.0 ** -60
        else:
            x[0, 5, 2] = 4096.0
    check('mxh_xin', edit, oracle_overflows=variant == 'outlier')


@pytest.mark.parametrize('j_bias', [0.0, 2.0])
@pytest.mark.parametrize('family', FAMILY_IDS)
def test_sigmoid_at_its_switch_over(family, j_bias):
    """(f) zero weights, x = 0: z = bias exactly.  Output-gate biases -80, -80.25 .. -95 on consecutive units, the other
    gates 0 (then c = 0 and out = 0 unless the gate is NaN), and with the tanh gate at 2 (c > 0: out = o tanh(c), a
    function of the one bias).  out is finite, not negative, does not grow as the bias falls and is within 2e-38 of the
    oracle — everything here is below 1e-34: a statement about NaN, sign and garbage, not digits"""
    B, T, D, H, _ = FAMILIES[family]
    sweep = -80.0 - 0.25 * np.arange(61)

    def edit(x, p, dout):
        x[:] = 0
        for d in ('fw', 'bw'):
            p[d + '_kernel'][:] = 0
            p[d + '_bias'][:] = 0
            p[d + '_bias'][GATE_J * H:(GATE_J + 1) * H] = j_bias
            p[d + '_bias'][GATE_O * H:GATE_O * H + 61] = sweep
    out, rout, dx, rdx, lens = check(family, edit, out_only=True)
    for lo in (0, H):
        o, r = out[:, :, lo:lo + 61], rout[:, :, lo:lo + 61]
        assert np.isfinite(o).all() and (o >= 0).all()
        assert np.abs(o).max() < 1e-34
        assert (o[:, :, 1:] <= o[:, :, :-1]).all()
        assert np.abs(o - r).max() < 2e-38
