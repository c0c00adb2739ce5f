"""CPU: the float64 restatement of the self-attention block (tests/self_attn_ref.py) against central differences."""
import numpy as np

from tests import self_attn_ref as R


def test_restatement_gradients_match_central_differences():
    rng = np.random.default_rng(8)
    B, T, D, H, FF = 3, 4, 4, 2, 6
    lens = np.array([4, 2, 0])
    shapes = dict(zip(R.NAMES, [(D,)] * 4 + [(D, 3 * D), (3 * D,), (D, D), (D,), (D, FF), (FF,), (FF, D), (D,)]))
    P = {n: rng.standard_normal(s) * 0.7 for n, s in shapes.items()}
    h, r = rng.standard_normal((B, T, D)), rng.standard_normal((B, T, D))
    out, cache = R.block_fwd(h, lens, P, H)
    G, dh = R.block_bwd(r, cache)
    assert np.all(cache[7][1, 2:] == 0) and np.all(cache[7][2] == 0)            # attention rows past a length

    def loss():
        return float((R.block_fwd(h, lens, P, H)[0] * r).sum())
    eps = 1e-6
    for arr, g in [(P[n], G[n]) for n in R.NAMES] + [(h, dh)]:
        num = np.zeros(arr.shape)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + eps
            up = loss()
            arr[i] = keep - eps
            num[i] = (up - loss()) / (2 * eps)
            arr[i] = keep
        np.testing.assert_allclose(g, num, rtol=1e-6, atol=1e-7)
