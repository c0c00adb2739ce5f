"""Timing of gradient accumulation on the device (numbatches_to_aggregate): (a) the two launches it adds,
nabu_clip_accumulate_f32 with and without an accumulator and nabu_adam_clip_step_acc, over the flat buffer of cfg2, next
to a device copy of the same buffer and to nabu_adam_clip_step as yardsticks; (b) one cfg2 update with
`numbatches_to_aggregate = 4` against four plain training steps on the same four batches.

Protocol (tools/weight_noise_bench.py): everything is warmed up, then the candidates are timed alternately, one call of
each per repetition, with device events around the call; medians are reported, with the spread of the repetitions.

    python tools/grad_accum_bench.py [--reps 50] [--updates 8] [--no-step] [--out profiles/grad_accum.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nabu_amd import ops as hip, recipes                                      # noqa: E402
from nabu_amd.neuralnetworks.trainers import trainer_factory                  # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402

A = 4
ADAM = (1e-3, 0.9, 0.999, 1e-8, 1.0)


def source():
    """the batch source of bench.py's cfg2 leg"""
    return SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=60, time_reduction=8, seed=4234)


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def trainer(**over):
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
    data = source()
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0), data


def launches(reps):
    tr, _ = trainer()
    tr._create_graph()
    tr._ensure_variables()
    tr._init_optimizer()
    flat, m, v = tr.flat, tr.adam_m, tr.adam_v
    kept = flat.clone()
    n = flat.numel()
    g = torch.randn(n, device=flat.device) * 2.0
    acc, out = torch.zeros_like(flat), torch.empty_like(flat)
    calls = {'clip_accumulate_first': (lambda: hip.clip_accumulate(acc, None, g, 1.0), 8),
             'clip_accumulate': (lambda: hip.clip_accumulate(out, acc, g, 1.0), 12),
             'adam_clip_step_acc': (lambda: hip.adam_clip_step_acc(flat, None, acc, g, m, v, *ADAM, 0.25), 32),
             'adam_clip_step': (lambda: hip.adam_clip_step(flat, g, m, v, *ADAM, 0.25), 28),
             'device_copy': (lambda: out.copy_(g), 8)}
    for _ in range(5):
        for fn, _ in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, (fn, _) in calls.items():
            times[k].append(timed_once(fn))
    flat.copy_(kept)
    row = {'workload': 'cfg2', 'flat_elements': n}
    for k, t in times.items():
        us = 1e3 * float(np.median(t))
        row[k + '_us'] = round(us, 2)
        row[k + '_min_max_us'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
        row[k + '_bytes_per_element'] = calls[k][1]
        row[k + '_gb_per_s'] = round(calls[k][1] * n / us / 1e3, 1)
    row['clip_accumulate_first_over_copy'] = round(row['clip_accumulate_first_us'] / row['device_copy_us'], 3)
    row['clip_accumulate_over_copy'] = round(row['clip_accumulate_us'] / row['device_copy_us'], 3)
    row['adam_acc_over_adam'] = round(row['adam_clip_step_acc_us'] / row['adam_clip_step_us'], 3)
    del tr
    torch.cuda.empty_cache()
    return row


def updates(n, warmup=2):
    """one accumulated update of A batches against A plain steps on the same resident batches, alternating"""
    acc_tr, data = trainer(**{'trainer.numbatches_to_aggregate': A})
    plain_tr, _ = trainer()
    batches = [acc_tr.to_device(data.batch(i)) for i in range(A)]

    def plain():
        for b in batches:
            plain_tr.step(b)
    runs = {'accumulated_update': lambda: acc_tr.step_accumulated(batches), 'plain_steps': plain}
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(n):
        for k, fn in runs.items():
            times[k].append(timed_once(fn))
    out = {'micro_batches': A, 'updates': n}
    for k, t in times.items():
        out[k + '_ms'] = round(float(np.median(t)), 3)
        out[k + '_min_max_ms'] = [round(min(t), 3), round(max(t), 3)]
    out['ratio'] = round(out['accumulated_update_ms'] / out['plain_steps_ms'], 4)
    # the margin: the spread between repetitions of the yardstick, relative to its median
    out['plain_spread'] = round((max(times['plain_steps']) - min(times['plain_steps'])) / out['plain_steps_ms'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--updates', type=int, default=8)
    ap.add_argument('--no-step', action='store_true', help='the launch timings only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_accum.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'grad_accum_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'grad_accum', 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'launches': launches(args.reps)}
    if not args.no_step:
        res['cfg2_update'] = updates(args.updates)
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
