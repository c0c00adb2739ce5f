"""Timing of the transducer's forced alignment (csrc/transducer_align.hip) against the transducer loss (csrc/transducer.hip)
IN THE SAME RUN on the same operands, at the shapes tools/transducer_bench.py uses:
    [32, 125, 40] with L ~ 40
    [32, 1000, 40] with L ~ 50
Per shape: the alignment's sweep-and-backtrace launch on its own (NABU_TRANSDUCER_ALIGN_LAUNCHES=2 on a workspace a
complete call has filled) against the loss's sweeps launch on its own (NABU_TRANSDUCER_LAUNCHES=2, likewise), and the
whole alignment call against the whole loss call.
The bar is on the launch: the alignment's takes no longer than the loss's sweeps launch at the same shape — that one is a
wave per sweep walking the same diagonals with add, exp, log, add on its chain, where the alignment has add and max and
then a backtrace of T_b + U_b steps.  The whole call's ratio is reported without a bar.

Protocol (tools/transducer_bench.py's): everything is warmed up; a round times the arms alternately, one call of each
per repetition, between device events, and keeps the median of each; medians of --rounds rounds are reported with the
spread of the rounds ((max - min) / median).

    python tools/transducer_align_bench.py [--reps 200] [--rounds 5] [--out profiles/transducer_align.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
from transducer_bench import SHAPES, operands, rounds_of  # noqa: E402

LOSS_SWITCH, ALIGN_SWITCH = 'NABU_TRANSDUCER_LAUNCHES', 'NABU_TRANSDUCER_ALIGN_LAUNCHES'


def only(switch, mask, everything, fn):
    """fn with the launch mask of `switch` set to `mask` for the call (both switches are read on every call)"""
    def run():
        os.environ[switch] = str(mask)
        try:
            return fn()
        finally:
            os.environ[switch] = str(everything)
    return run


def measure(shape, reps, rounds):
    from nabu_amd import ops
    dev = torch.device('cuda')
    f, g, enc_len, labels, label_len = operands(shape, dev)
    B, T, C = f.shape
    U1 = g.shape[1]

    def loss():
        return ops.transducer_loss_grad(f, g, enc_len, labels, label_len, 1.0 / B)

    def align():
        return ops.transducer_align(f, g, enc_len, labels, label_len)
    arms = {'align_launch': only(ALIGN_SWITCH, 2, 3, align), 'loss_sweeps': only(LOSS_SWITCH, 2, 7, loss),
            'align': align, 'loss': loss}
    ref_loss, ref_align = loss(), align()
    assert int(ref_loss[3].item()) == 0 and int(ref_align[4].item()) == 0
    # each launch alone, on the workspace its complete call filled: the same results
    assert torch.equal(arms['loss_sweeps']()[0], ref_loss[0])
    again = arms['align_launch']()
    assert all(torch.equal(a, r) for a, r in zip(again, ref_align))
    assert bool((ref_align[3] <= -ref_loss[0] + 1e-3 * ref_loss[0].abs()).all())        # best path <= all paths
    for _ in range(10):
        for fn in arms.values():
            fn()
    per_round, med, spread = rounds_of(arms, reps, rounds)
    return {'shape': dict(shape, U1=U1), 'us_per_round': per_round, 'median_us': med, 'spread': spread,
            'align_launch_over_loss_sweeps': round(med['align_launch'] / med['loss_sweeps'], 4), 'bar': 1.0,
            'bar_met': bool(med['align_launch'] <= med['loss_sweeps']),
            'align_over_loss': round(med['align'] / med['loss'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transducer_align.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'transducer_align_bench needs a GPU'
    torch.cuda.set_device(0)
    route = 'workgroup' if os.environ.get('NABU_TRANSDUCER_ALIGN_WORKGROUP', '0') not in ('', '0') else 'default'
    res = {'bench': 'transducer_align', 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'route': route, 'cases': [measure(s, args.reps, args.rounds) for s in SHAPES]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
