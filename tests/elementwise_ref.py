"""NumPy restatements of the small kernels that oracle/nabu_oracle.py does not have, written from the formulas.  Every
function takes a dtype and does ALL its arithmetic in it: float64 is the reference, float32 on the same inputs is the
error a single-precision evaluation is entitled to (tests/test_hip_elementwise.py compares the device with four times
that).  layer_norm_fwd/bwd, relu_fwd/bwd and pyramid_stack_fwd/bwd are the oracle's and are not repeated here.

The Speller's LSTM cell for ONE step (tf.contrib.rnn.LSTMCell: gate column blocks i, j, f, o; forget bias 1):

    z += bias (+ emb[ids[b]]: a one-hot input times the kernel is one row of it)
    i, g, f, o = sigmoid(z_i), tanh(z_j), sigmoid(z_f + 1), sigmoid(z_o)
    c' = c f + i g,   h' = tanh(c') o

and a FINISHED row (step >= seq_len[b]: dynamic_decode's impute_finished) keeps c and h, has zero activations, a
zero dz and hands dc through unchanged."""
import numpy as np


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return 1 / (1 + np.exp(-x))


def lstm_cell_fwd(step, seq_len, z, bias, c_prev, h_prev, emb=None, ids=None, dtype=np.float64):
    """(acts [B,4U], c_new [B,U], h_new [B,U]); z [B,4U] is the step product WITHOUT the bias, emb [C,4U] / ids [B] the
    optional one-hot input"""
    z, bias, c_prev, h_prev = (np.asarray(a, dtype) for a in (z, bias, c_prev, h_prev))
    U = c_prev.shape[1]
    live = (step < np.asarray(seq_len))[:, None]
    z = z + bias[None, :]
    if emb is not None:
        z = z + np.asarray(emb, dtype)[np.asarray(ids)]
    one = dtype(1)
    i, g = _sigmoid(z[:, :U]), np.tanh(z[:, U:2 * U])
    f, o = _sigmoid(z[:, 2 * U:3 * U] + one), _sigmoid(z[:, 3 * U:])
    c = c_prev * f + i * g
    h = np.tanh(c) * o
    acts = np.where(live, np.concatenate([i, g, f, o], 1), dtype(0))
    return acts.astype(dtype), np.where(live, c, c_prev).astype(dtype), np.where(live, h, h_prev).astype(dtype)


def lstm_cell_bwd(step, seq_len, acts, c_new, c_prev, dh, dc_in, dh2=None, dtype=np.float64):
    """(dz [B,4U], dc_out [B,U]) from the step's stored activations and states; dh2: a second gradient of h (added)"""
    acts, c_new, c_prev, dh, dc_in = (np.asarray(a, dtype) for a in (acts, c_new, c_prev, dh, dc_in))
    U = c_prev.shape[1]
    live = (step < np.asarray(seq_len))[:, None]
    one = dtype(1)
    i, g, f, o = acts[:, :U], acts[:, U:2 * U], acts[:, 2 * U:3 * U], acts[:, 3 * U:]
    tc = np.tanh(c_new)
    dht = dh if dh2 is None else dh + np.asarray(dh2, dtype)
    dct = dc_in + dht * o * (one - tc * tc)
    dz = np.concatenate([dct * g * i * (one - i), dct * i * (one - g * g), dct * c_prev * f * (one - f),
                         dht * tc * o * (one - o)], 1)
    return np.where(live, dz, dtype(0)).astype(dtype), np.where(live, dct * f, dc_in).astype(dtype)


def clip(x, bound, dtype=np.float64):
    """tf.clip_by_value(x, -bound, bound): a NaN stays a NaN (the TF kernels compare, they do not pick the number)"""
    x = np.asarray(x, dtype)
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, dtype(-bound)), dtype(bound))).astype(dtype)


def sum_tree(x, scale=1.0, dtype=np.float64):
    """scale * sum(x) in the shape nabu_sum_f32 adds it: 256 serial chains (chain t takes x[t], x[t + 256], ...), then
    an 8-level tree that folds the upper half onto the lower.  In float32 this is the kernel's own result, bit for
    bit (IEEE additions in a fixed order); in float64 it is the sum."""
    x = np.asarray(x, dtype).reshape(-1)
    rows = -(-x.size // 256)
    padded = np.zeros(max(rows, 1) * 256, dtype)
    padded[:x.size] = x
    s = np.zeros(256, dtype)
    for row in padded.reshape(-1, 256):
        s = s + row
    o = 128
    while o >= 1:
        s = s[:o] + s[o:2 * o]
        o //= 2
    return dtype(scale) * s[0]
