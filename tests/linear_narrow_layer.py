"""dnn_decoder.linear forward + backward at B*T = 66, F = 40, C = 9 on seeded inputs -> {name: array}.  Imported by
tests/test_hip_linear_narrow.py, and run by it as a program (`python linear_narrow_layer.py OUT.npz`) in a process of its
own with NABU_LINEAR_NARROW=0: the switch is read once per process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, F, C = 2, 33, 40, 9


def inputs():
    rng = np.random.default_rng(66)
    return (rng.standard_normal((B, T, F)).astype(np.float32), rng.standard_normal((B, T, C)).astype(np.float32),
            rng.standard_normal(C).astype(np.float32))


def run():
    import torch
    from nabu_amd import variables as vs
    from nabu_amd.autodiff import Tape, record
    from nabu_amd.neuralnetworks.models.ed_decoders import dnn_decoder
    x_h, dout_h, b_h = inputs()
    x, dout = torch.tensor(x_h, device='cuda'), torch.tensor(dout_h, device='cuda')
    store = vs.VariableStore(seed=5)
    got = {}
    with vs.as_default(store), Tape() as tape:
        src = torch.zeros(1, device='cuda')
        record([src], [x], lambda g: got.update(dx=g) or [None])       # x is a layer's output: the linear map owes it a gradient
        with vs.variable_scope('outlayer'):
            vs.get_variable('biases', [C], vs.zeros).data.copy_(torch.tensor(b_h))
        out = dnn_decoder.linear(x, C, 'outlayer')
        root = torch.zeros((), device='cuda')
        record([out], [root], lambda g: [dout])
        tape.backward(root)
    torch.cuda.synchronize()
    W, b = store.vars['outlayer/weights'], store.vars['outlayer/biases']
    return {'out': out.cpu().numpy(), 'dx': got['dx'].cpu().numpy(), 'dW': W.grad.cpu().numpy(), 'db': b.grad.cpu().numpy(),
            'W': W.data.cpu().numpy(), 'b': b.data.cpu().numpy()}


if __name__ == '__main__':
    np.savez(sys.argv[1], **run())
    print('LAYER OK')
