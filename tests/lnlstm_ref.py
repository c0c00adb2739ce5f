"""NumPy restatement of a layer-normalised BLSTM layer: tf.contrib.rnn.LayerNormBasicLSTMCell(num_units,
layer_norm=True) under bidirectional_dynamic_rnn with ragged lengths, forward and hand-written backward.  Written
from the cell's description (include/nabu_hip.h states the same), not from the kernels; it evaluates in the dtype of
its arguments (float64: the reference; float32: the yardstick of the kernel's error).

Per direction, batch row b and step s < len[b]:
    z = [x_t, h] . kernel                                   (no bias)
    LN_k(v) = gamma_k (v - mean v) / sqrt(var v + 1e-12) + beta_k     per gate, over its H units, biased variance
    c' = c sigmoid(LN_f(z_f) + 1) + sigmoid(LN_i(z_i)) tanh(LN_j(z_j));   c = LN_state(c');   h = tanh(c) sigmoid(LN_o(z_o))
steps s >= len[b]: output 0, state frozen; the backward direction runs over the reversed valid part.
The norms are oracle.nabu_oracle.layer_norm_fwd / layer_norm_bwd on [B, H] arrays (moments per row)."""
import numpy as np

from oracle import nabu_oracle as O

SCOPES = ('input', 'transform', 'forget', 'output', 'state')
CELL = 'bidirectional_rnn/%s/layer_norm_basic_lstm_cell'


def variable_shapes(D, H):
    """ordered (name relative to the layer's scope, shape) of both directions' variables: kernel, then gamma / beta of
    the five norm scopes; there is no bias"""
    out = []
    for d in ('fw', 'bw'):
        cell = CELL % d
        out.append((cell + '/kernel', (D + H, 4 * H)))
        for s in SCOPES:
            out += [('%s/%s/gamma' % (cell, s), (H,)), ('%s/%s/beta' % (cell, s), (H,))]
    return out


def init_params(rng, D, H, dtype=np.float64, perturb=0.0):
    """{fw,bw}_{kernel,gamma,beta}: Glorot kernel, gamma = 1, beta = 0 (+ perturb * N(0,1): a trained layer)"""
    p = {}
    for d in ('fw', 'bw'):
        p[d + '_kernel'] = O.glorot_uniform(rng, (D + H, 4 * H)).astype(dtype)
        p[d + '_gamma'] = (1.0 + perturb * rng.standard_normal((5, H))).astype(dtype)
        p[d + '_beta'] = (perturb * rng.standard_normal((5, H))).astype(dtype)
    return p


def cast(p, dtype):
    return {k: v.astype(dtype) for k, v in p.items()}


def dir_fwd(x, lens, kernel, gamma, beta, reverse):
    """one direction.  x [B,T,D], kernel [(D+H),4H] (gate column blocks i, j, f, o), gamma / beta [5,H] (SCOPES order).
    Returns out [B,T,H] and the cache of dir_bwd; cache['min_var'] = the smallest variance any norm saw."""
    B, T, D = x.shape
    H = kernel.shape[1] // 4
    dt = x.dtype
    Wx, Wh = kernel[:D], kernel[D:]
    out = np.zeros((B, T, H), dt)
    h = np.zeros((B, H), dt)
    c = np.zeros((B, H), dt)
    lens = np.asarray(lens)
    ar = np.arange(B)
    steps = []
    min_var = np.inf
    for s in range(int(lens.max()) if B else 0):
        act = s < lens
        t = np.where(act, np.where(reverse, lens - 1 - s, s), 0)
        z = x[ar, t] @ Wx + h @ Wh
        y, lnc = [], []
        for k in range(4):
            yk, ck = O.layer_norm_fwd(z[:, k * H:(k + 1) * H], gamma[k], beta[k])
            y.append(yk)
            lnc.append(ck)
        i, g, f, o = O.sigmoid(y[0]), np.tanh(y[1]), O.sigmoid(y[2] + O.FORGET_BIAS), O.sigmoid(y[3])
        craw = c * f + i * g
        cn, cc = O.layer_norm_fwd(craw, gamma[4], beta[4])
        lnc.append(cc)
        hn = np.tanh(cn) * o
        for ck in lnc:
            var = 1.0 / np.square(ck[1].astype(np.float64)) - 1e-12
            min_var = min(min_var, float(var[act].min()))
        ia = np.nonzero(act)[0]
        out[ia, t[ia]] = hn[ia]
        steps.append(dict(act=act, t=t, i=i, g=g, f=f, o=o, cn=cn, cprev=c, hprev=h, ln=lnc))
        a = act[:, None]
        c = np.where(a, cn, c)
        h = np.where(a, hn, h)
    return out, dict(x=x, kernel=kernel, steps=steps, min_var=min_var)


def dir_bwd(dout, cache):
    """gradient of dir_fwd.  dout [B,T,H] (rows past len are ignored).  Returns dx, dkernel, dgamma [5,H], dbeta [5,H]"""
    x, kernel, steps = cache['x'], cache['kernel'], cache['steps']
    B, T, D = x.shape
    H = kernel.shape[1] // 4
    dt = x.dtype
    Wx, Wh = kernel[:D], kernel[D:]
    dx = np.zeros_like(x)
    dkernel = np.zeros_like(kernel)
    dgamma, dbeta = np.zeros((5, H), dt), np.zeros((5, H), dt)
    dh = np.zeros((B, H), dt)
    dc = np.zeros((B, H), dt)
    ar = np.arange(B)
    for st in reversed(steps):
        a, t = st['act'][:, None], st['t']
        i, g, f, o = st['i'], st['g'], st['f'], st['o']
        tc = np.tanh(st['cn'])
        dht = np.where(a, dout[ar, t] + dh, 0)            # a finished row takes no part in this step
        dcn = np.where(a, dc + dht * o * (1 - tc * tc), 0)
        dcraw, dg_, db_ = O.layer_norm_bwd(dcn, st['ln'][4])
        dgamma[4] += dg_
        dbeta[4] += db_
        dy = [dcraw * g * i * (1 - i), dcraw * i * (1 - g * g), dcraw * st['cprev'] * f * (1 - f), dht * tc * o * (1 - o)]
        dz = []
        for k in range(4):
            dzk, dg_, db_ = O.layer_norm_bwd(dy[k], st['ln'][k])
            dz.append(dzk)
            dgamma[k] += dg_
            dbeta[k] += db_
        dz = np.concatenate(dz, 1)                         # rows of finished sequences are exactly 0
        ia = np.nonzero(st['act'])[0]
        dx[ia, t[ia]] = (dz @ Wx.T)[ia]
        dkernel += np.concatenate([x[ar, t], st['hprev']], 1).T @ dz
        dh = np.where(a, dz @ Wh.T, dh)
        dc = np.where(a, dcraw * f, dc)
    return dx, dkernel, dgamma, dbeta


def blstm_fwd(x, lens, p):
    """p = dict({fw,bw}_{kernel,gamma,beta}); out [B,T,2H] = concat(fw, bw)"""
    of, cf = dir_fwd(x, lens, p['fw_kernel'], p['fw_gamma'], p['fw_beta'], False)
    ob, cb = dir_fwd(x, lens, p['bw_kernel'], p['bw_gamma'], p['bw_beta'], True)
    return np.concatenate([of, ob], 2), (cf, cb)


def blstm_bwd(dout, cache):
    cf, cb = cache
    H = dout.shape[2] // 2
    dxf, dkf, dgf, dbf = dir_bwd(dout[:, :, :H], cf)
    dxb, dkb, dgb, dbb = dir_bwd(dout[:, :, H:], cb)
    return dxf + dxb, dict(fw_kernel=dkf, fw_gamma=dgf, fw_beta=dbf, bw_kernel=dkb, bw_gamma=dgb, bw_beta=dbb)


def min_variance(cache):
    return min(cache[0]['min_var'], cache[1]['min_var'])


# -- encoders (the layer-normalised twins of oracle.nabu_oracle.listener_* / dblstm_*, no regularisation) -------------
def listener_fwd(x, lens, layers, pyramid_steps=2):
    caches = []
    h, l = x, np.asarray(lens)
    for p in layers[:-1]:
        o, c = blstm_fwd(h, l, p)
        caches.append((c, o.shape[1]))
        h, l = O.pyramid_stack_fwd(o, l, pyramid_steps)
    o, c = blstm_fwd(h, l, layers[-1])
    caches.append((c, o.shape[1]))
    return o, l, caches


def listener_bwd(dout, caches, pyramid_steps=2):
    d, g = blstm_bwd(dout, caches[-1][0])
    grads = [g]
    for c, T in reversed(caches[:-1]):
        d, g = blstm_bwd(O.pyramid_stack_bwd(d, T, pyramid_steps), c)
        grads.append(g)
    return d, grads[::-1]


def dblstm_fwd(x, lens, layers):
    caches = []
    h = x
    for p in layers:
        h, c = blstm_fwd(h, lens, p)
        caches.append(c)
    return h, np.asarray(lens), caches


def dblstm_bwd(dout, caches):
    grads = []
    d = dout
    for c in reversed(caches):
        d, g = blstm_bwd(d, c)
        grads.append(g)
    return d, grads[::-1]
