"""CPU: the float64 restatement of the convolutional front end (tests/conv_ref.py) against central differences."""
import numpy as np

from tests import conv_ref as R


def test_restatement_gradients_match_central_differences():
    rng = np.random.default_rng(5)
    B, T, D, blocks, C = 2, 5, 6, 2, 2
    lens = np.array([5, 3])
    x = rng.standard_normal((B, T, D))
    params = [[rng.standard_normal(s) * 0.5 for s in ((3, 3, blocks, C), (C,), (3, 3, C, C), (C,))]]
    out, out_lens, caches = R.frontend_fwd(x, lens, params, blocks)
    assert out.shape == (B, 3, 2 * C) and list(out_lens) == [3, 2]
    r = rng.standard_normal(out.shape)
    grads, dx = R.frontend_bwd(r, caches)

    def loss():
        return float((R.frontend_fwd(x, lens, params, blocks)[0] * r).sum())
    eps = 1e-6
    for arr, g in list(zip(params[0], grads[0])) + [(x, dx.transpose(0, 1, 3, 2).reshape(x.shape))]:
        num = np.zeros(arr.shape)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + eps
            up = loss()
            arr[i] = keep - eps
            num[i] = (up - loss()) / (2 * eps)
            arr[i] = keep
        np.testing.assert_allclose(g, num, rtol=1e-6, atol=1e-7)
