"""What tests/test_hip_transducer.py runs on its cases; importable without a GPU.

As a program (a child process started with NABU_TRANSDUCER_WORKGROUP=1, which csrc/transducer.hip reads once per
process) it runs every shape the wave route takes on the workgroup route and saves nll, df, dg and status of each to
an .npz: the parent compares them with the bits its own, default-route run produced.
usage: python tests/transducer_check.py OUT.npz"""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

from tests import ctc_cases as cc  # noqa: E402
from tests import transducer_cases as tc  # noqa: E402

ENTRIES = [(s, r) for s in tc.ALL_SHAPES for r in cc.REGIMES]
_cases = {}


def entry_id(entry):
    return '%dx%dx%dx%d-%s' % (entry[0] + (entry[1],))


def case_of(entry):
    """the case of an entry, built once (its float64 and float32 references are kept with it)"""
    key = entry_id(entry)
    if key not in _cases:
        shape, regime = entry
        _cases[key] = tc.make_case(*shape, regime=regime, seed=tc.seed_of(*shape))
    return _cases[key]


def forced_workgroup():
    return os.environ.get('NABU_TRANSDUCER_WORKGROUP', '0') not in ('', '0')


def run(case, grad_scale=1.0):
    """one call of ops.transducer_loss_grad on host arrays -> (nll, df, dg, status) as NumPy arrays (status an int)"""
    import torch
    from nabu_amd import ops

    def dev(a, dtype):
        return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()
    f, g, enc_len, labels, label_len = case
    nll, df, dg, status = ops.transducer_loss_grad(dev(f, torch.float32), dev(g, torch.float32), dev(enc_len, torch.int32),
                                                   dev(labels, torch.int32) if labels.size else None,
                                                   dev(label_len, torch.int32), grad_scale)
    return nll.cpu().numpy(), df.cpu().numpy(), dg.cpu().numpy(), int(status.item())


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)) for x, y in zip(a, b))


def main(argv):
    assert forced_workgroup(), 'run with NABU_TRANSDUCER_WORKGROUP=1'
    saved = {}
    for entry in ENTRIES:
        if not tc.wave_eligible(entry[0][3]):
            continue
        out = run(case_of(entry))
        for name, a in zip(('nll', 'df', 'dg', 'status'), out):
            saved['%s/%s' % (entry_id(entry), name)] = np.asarray(a)
        print('CASE %s workgroup status %d' % (entry_id(entry), out[3]), flush=True)
    np.savez(argv[0], **saved)
    print('TRANSDUCER DONE %d arrays' % len(saved))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
