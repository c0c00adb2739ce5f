"""Float64 restatement of global-norm gradient clipping (the [trainer] key clip_gradient_norm), shared by
tests/test_grad_norm.py (CPU) and tests/test_hip_grad_norm.py (GPU).  NumPy only; nothing here calls the package."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


def global_norm(x):
    """the L2 norm of the whole (flat or listed) gradient, every term squared and summed in float64"""
    parts = x if isinstance(x, (list, tuple)) else [x]
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(p, np.float64)))) for p in parts)))


def mean_gradient(grads):
    """the gradient an update applies before clipping: the plain mean of its A * world micro-batch gradients (the
    accumulated and the data-parallel mean are the same expression), nothing clipped per element"""
    return np.mean([np.asarray(g, np.float64) for g in grads], 0)


def factor_f32(norm, scale, max_norm):
    """what the device multiplies the gradient SUM by, in float32 and in the order the kernel states:
    norm > max_norm ? scale * (max_norm / norm) : scale, NaN when the norm is NaN or inf"""
    norm, scale, max_norm = np.float32(norm), np.float32(scale), np.float32(max_norm)
    if not np.isfinite(norm):
        return np.float32(np.nan)
    with np.errstate(all='ignore'):
        return scale * (max_norm / norm) if norm > max_norm else scale


def stats(x, scale, max_norm):
    """(norm as float32, factor as float32, skipped as 0 | 1) of the gradient sum x with the mean's scale"""
    with np.errstate(all='ignore'):
        norm = np.float32(np.float64(np.float32(scale)) * global_norm(x))
    return norm, factor_f32(norm, scale, max_norm), int(not np.isfinite(norm))


def clipped(mean, max_norm):
    """mean * min(1, max_norm / ||mean||) in float64, or None when the norm is not finite (the update is skipped)"""
    mean = np.asarray(mean, np.float64)
    with np.errstate(all='ignore'):
        norm = global_norm(mean)
    if not np.isfinite(norm):
        return None
    return mean * (max_norm / norm) if norm > max_norm else mean


def adam_update(theta, g, m, v, t, lr):
    """TF-style Adam on g as it is (no clamp): oracle.nabu_oracle.clip_adam_update without its clip"""
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    lr_t = lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    return theta - lr_t * m / (np.sqrt(v) + EPS), m, v


def update(theta, grads, m, v, t, lr, max_norm, clean=None):
    """one update with clip_gradient_norm = max_norm on the micro-batch gradients `grads` (a list, or a list of lists of
    per-variable arrays is NOT taken: flatten first): Adam on the norm-clipped mean.  A mean whose norm is not finite
    skips the update: m and v are returned as they are and theta too — or `clean`, the parameters before a weight-noise
    step, when given.  t still counts the skipped update (the host's adam_step advances).  -> (theta, m, v, norm)"""
    mean = mean_gradient(grads)
    with np.errstate(all='ignore'):
        norm = global_norm(mean)
    start = theta if clean is None else clean
    g = clipped(mean, max_norm)
    if g is None:
        return np.array(start, np.float64), m, v, norm
    return adam_update(np.asarray(start, np.float64), g, m, v, t, lr) + (norm,)
