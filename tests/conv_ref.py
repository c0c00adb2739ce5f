"""float64 restatement of the convolutional front end (conv2d.hip): channels-last x [B,T,F,C], frames >= len read as zero and
are zero in every result.  Error bounds are the same functions on absolute values: conv(|x|, lens, |w|, |bias|, relu=False)."""
import numpy as np


def gamma(n, u=2.0 ** -24):
    return n * u / (1 - n * u)


def _taps(xb, L, F):         # the nine shifted views of one utterance's valid frames, zero padded: [(kt, kf, [L,F,C])]
    xp = np.pad(xb[:L], ((1, 1), (1, 1), (0, 0)))
    return [(kt, kf, xp[kt:kt + L, kf:kf + F]) for kt in range(3) for kf in range(3)]


def conv(x, lens, w, bias=None, relu=True):
    B, T, F, _ = x.shape
    y = np.zeros((B, T, F, w.shape[3]))
    for b, L in enumerate(np.clip(lens, 0, T)):
        for kt, kf, v in _taps(x[b], L, F):
            y[b, :L] += v @ w[kt, kf]
        if bias is not None:
            y[b, :L] += bias
    return np.maximum(y, 0) if relu else y


def flip(w):
    return w[::-1, ::-1].transpose(0, 1, 3, 2)


def wgrad(x, lens, g):
    """(dw, dbias) for g = dy * (y > 0)"""
    B, T, F, _ = x.shape
    dw = np.zeros((3, 3, x.shape[3], g.shape[3]))
    db = np.zeros(g.shape[3])
    for b, L in enumerate(np.clip(lens, 0, T)):
        for kt, kf, v in _taps(x[b], L, F):
            dw[kt, kf] += np.einsum('tfc,tfd->cd', v, g[b, :L])
        db += g[b, :L].sum((0, 1))
    return dw, db


def _windows(x, lens):
    B, T, F, _ = x.shape
    for b, L in enumerate(np.clip(lens, 0, T)):
        for tp in range((L + 1) // 2):
            for fp in range((F + 1) // 2):
                yield b, tp, fp, x[b, 2 * tp:min(2 * tp + 2, L), 2 * fp:2 * fp + 2]


def pool(x, lens):
    B, T, F, C = x.shape
    y = np.zeros((B, (T + 1) // 2, (F + 1) // 2, C), x.dtype)
    for b, tp, fp, win in _windows(x, lens):
        y[b, tp, fp] = win.max((0, 1))
    return y


def pool_bwd(x, lens, dy):
    """the gradient goes to the first maximum of a window in (t, f) order (np.argmax's choice)"""
    dx = np.zeros(x.shape, dy.dtype)
    for b, tp, fp, win in _windows(x, lens):
        arg = win.reshape(-1, win.shape[2]).argmax(0)
        for c, a in enumerate(arg):
            dx[b, 2 * tp + a // win.shape[1], 2 * fp + a % win.shape[1], c] = dy[b, tp, fp, c]
    return dx


def frontend_fwd(x, lens, params, blocks):
    """x [B,T,D] with `blocks` equal column blocks as channels; params: [(w0, b0, w1, b1)] per conv block.
    Returns ([B,T'',F''*C], lengths, caches)."""
    B, T, D = x.shape
    h = x.reshape(B, T, blocks, D // blocks).transpose(0, 1, 3, 2)
    caches = []
    for w0, b0, w1, b1 in params:
        y0 = conv(h, lens, w0, b0)
        y1 = conv(y0, lens, w1, b1)
        caches.append((h, lens, y0, y1, w0, w1))
        h, lens = pool(y1, lens), -(-np.clip(lens, 0, h.shape[1]) // 2)
    return h.reshape(h.shape[0], h.shape[1], -1), lens, caches


def frontend_bwd(dout, caches):
    """gradients [(dw0, db0, dw1, db1)] per block and the gradient at the channels-last input of the first block"""
    grads = []
    for h, lens, y0, y1, w0, w1 in reversed(caches):
        g1 = pool_bwd(y1, lens, dout.reshape((y1.shape[0], (y1.shape[1] + 1) // 2, (y1.shape[2] + 1) // 2, y1.shape[3])))
        g1 = g1 * (y1 > 0)
        dw1, db1 = wgrad(y0, lens, g1)
        g0 = conv(g1, lens, flip(w1), relu=False) * (y0 > 0)
        dw0, db0 = wgrad(h, lens, g0)
        dout = conv(g0, lens, flip(w0), relu=False)
        grads.insert(0, (dw0, db0, dw1, db1))
    return grads, dout
