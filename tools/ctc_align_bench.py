"""Timing of forced alignment (nabu_ctc_align) against the CTC loss launch (nabu_ctc_loss_grad) IN THE SAME RUN ON THE
SAME OPERANDS, at the two shapes the recipes train at:
    [32, 125, 40] with L ~ 40   (cfg2: the Listener's output; the loss takes its split wave kernel)
    [32, 1000, 40] with L ~ 50  (cfg1: the loss takes its workgroup kernel, alignment the wave route)
The bar is the loss launch at the same shape: alignment — one sweep of add and max — takes no longer than two sweeps
of log-sum-exp plus a [B,T,C] gradient write.

Protocol: everything is warmed up; a round times the two calls alternately, one of each per repetition, between
device events, and keeps the median of each; medians of --rounds rounds are reported with the spread of the rounds
((max - min) / median).  NABU_CTC_ALIGN_WORKGROUP=1 in the environment times the workgroup route instead.

    python tools/ctc_align_bench.py [--reps 50] [--rounds 5] [--out profiles/ctc_align.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [dict(B=32, T=125, C=40, L=40), dict(B=32, T=1000, C=40, L=50)]


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def operands(shape, dev):
    """seeded logits N(0, 2), full-length utterances, label lengths within 10 % of L"""
    B, T, C, L = shape['B'], shape['T'], shape['C'], shape['L']
    rng = np.random.default_rng(1000 * T + L)
    Lmax = L + L // 10
    label_len = rng.integers(L - L // 10, Lmax + 1, B).astype(np.int32)
    labels = rng.integers(0, C - 1, (B, Lmax)).astype(np.int32)
    logits = (2.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    return (torch.tensor(logits, device=dev), torch.full((B,), T, dtype=torch.int32, device=dev),
            torch.tensor(labels, device=dev), torch.tensor(label_len, device=dev))


def measure(shape, reps, rounds):
    from nabu_amd import ops
    dev = torch.device('cuda')
    logits, logit_len, labels, label_len = operands(shape, dev)
    arms = {'align': lambda: ops.ctc_align(logits, logit_len, labels, label_len),
            'loss': lambda: ops.ctc_loss_grad(logits, logit_len, labels, label_len, 1.0 / shape['B'])}
    assert int(arms['align']()[4].item()) == 0 and int(arms['loss']()[2].item()) == 0
    for _ in range(10):
        for fn in arms.values():
            fn()
    per_round = {k: [] for k in arms}
    for _ in range(rounds):
        t = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                t[k].append(timed_once(fn))
        for k in arms:
            per_round[k].append(1e3 * float(np.median(t[k])))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    return {'shape': shape, 'us_per_round': {k: [round(x, 2) for x in v] for k, v in per_round.items()},
            'median_us': {k: round(v, 2) for k, v in med.items()},
            'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in per_round.items()},
            'align_over_loss': round(med['align'] / med['loss'], 4), 'bar_met': bool(med['align'] <= med['loss'])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctc_align.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ctc_align_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, ROOT)
    res = {'bench': 'ctc_align', 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'route': 'workgroup' if os.environ.get('NABU_CTC_ALIGN_WORKGROUP', '0') not in ('', '0') else 'default',
           'cases': [measure(s, args.reps, args.rounds) for s in SHAPES]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
