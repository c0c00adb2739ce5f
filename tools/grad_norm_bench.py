"""Timing of global-norm gradient clipping on the device (clip_gradient_norm): (a) the launches it adds over the flat
buffer of cfg2 — nabu_grad_norm_f32 without and with an accumulator (two launches inside each call) and
nabu_adam_scaled_step — next to a device copy of the same buffer, which is the bar for the reduction (it reads 4 or 8
bytes per parameter, the copy reads 4 and writes 4), and to nabu_adam_clip_step; (b) the cfg2 training step with the key
set against the step without it.

Protocol (tools/grad_accum_bench.py): everything is warmed up, then the candidates are timed alternately, one call of each
per repetition, with device events around the call; medians are reported, with the spread of the repetitions.  The two
reductions alternate with the copy, the two Adam launches with each other.  The steps
run in child processes, one per measurement, alternating without / with the key for --rounds rounds.  With
--parent-root DIR (a checkout of the parent commit with its library built) the step without the key is that checkout's;
otherwise it is this tree's and the result says so.

    python tools/grad_norm_bench.py [--reps 50] [--steps 30] [--rounds 2] [--parent-root DIR] [--no-step]
                                    [--out profiles/grad_norm.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAM = (1e-3, 0.9, 0.999, 1e-8)
CLIP_NORM = 1.0


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def trainer(**over):
    """a cfg2 trainer on the batch source of bench.py's cfg2 leg (the package comes from sys.path[0])"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
    data = SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=60, time_reduction=8, seed=4234)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0), data


def launches(reps):
    from nabu_amd import ops as hip
    tr, _ = trainer()
    tr._create_graph()
    tr._ensure_variables()
    tr._init_optimizer()
    flat, m, v = tr.flat, tr.adam_m, tr.adam_v
    kept = flat.clone()
    n = flat.numel()
    g = torch.randn(n, device=flat.device) * 2.0
    acc, out = torch.randn(n, device=flat.device), torch.empty_like(flat)
    stats, ws = hip.grad_norm_buffers(n, flat.device)
    hip.grad_norm(g, None, 0.25, 1e30, stats, ws)               # a finite factor for the scaled step (nothing is clipped)
    calls = {'grad_norm': (lambda: hip.grad_norm(g, None, 0.25, 1e30, stats, ws), 4),
             'grad_norm_acc': (lambda: hip.grad_norm(g, acc, 0.25, 1e30, stats, ws), 8),
             'adam_scaled_step': (lambda: hip.adam_scaled_step(flat, None, None, g, m, v, *ADAM, stats), 28),
             'adam_clip_step': (lambda: hip.adam_clip_step(flat, g, m, v, *ADAM, 1.0, 0.25), 28),
             'device_copy': (lambda: out.copy_(g), 8)}
    for _ in range(5):
        for fn, _ in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    # two alternations, so that each candidate runs behind its yardstick and the yardstick behind it: what the previous
    # launch left in the 256 MiB cache is worth more than 10 % on these launches (g alone is 135 MB)
    for group in (('grad_norm', 'grad_norm_acc', 'device_copy'), ('adam_scaled_step', 'adam_clip_step')):
        for _ in range(reps):
            for k in group:
                times[k].append(timed_once(calls[k][0]))
    flat.copy_(kept)
    norm, factor, skipped = hip.read_grad_stats(stats)
    row = {'workload': 'cfg2', 'flat_elements': n, 'norm': norm, 'factor': factor, 'skipped': skipped}
    for k, t in times.items():
        us = 1e3 * float(np.median(t))
        row[k + '_us'] = round(us, 2)
        row[k + '_min_max_us'] = [round(1e3 * min(t), 2), round(1e3 * max(t), 2)]
        row[k + '_bytes_per_element'] = calls[k][1]
        row[k + '_gb_per_s'] = round(calls[k][1] * n / us / 1e3, 1)
    row['grad_norm_over_copy'] = round(row['grad_norm_us'] / row['device_copy_us'], 3)
    row['grad_norm_acc_over_copy'] = round(row['grad_norm_acc_us'] / row['device_copy_us'], 3)
    row['reduction_within_the_copy_bar'] = bool(row['grad_norm_us'] <= row['device_copy_us']
                                                and row['grad_norm_acc_us'] <= row['device_copy_us'])
    row['adam_scaled_over_adam'] = round(row['adam_scaled_step_us'] / row['adam_clip_step_us'], 3)
    del tr
    torch.cuda.empty_cache()
    return row


def step_child(clip_norm, steps, warmup=3):
    """in a child process: `steps` training steps of cfg2 on one resident batch, each between two device events"""
    tr, data = trainer(**({'trainer.clip_gradient_norm': clip_norm} if clip_norm else {}))
    batch = tr.to_device(data.batch(0))
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    t = [timed_once(lambda: tr.step(batch)) for _ in range(steps)]
    out = {'clip_gradient_norm': clip_norm, 'steps': steps, 'step_ms': round(float(np.median(t)), 4),
           'min_max_ms': [round(min(t), 4), round(max(t), 4)]}
    if clip_norm:
        out['grad_stats'] = list(tr.grad_stats())
    print('STEP ' + json.dumps(out), flush=True)


def run_child(root, clip_norm, steps):
    cmd = [sys.executable, os.path.abspath(__file__), '--step-child', '--root', root, '--clip', repr(clip_norm),
           '--steps', str(steps)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in res.stdout.splitlines() if l.startswith('STEP ')]
    if res.returncode != 0 or not lines:
        raise RuntimeError('step measurement failed (%d): %s' % (res.returncode, res.stdout[-2000:]))
    return json.loads(lines[-1][5:])


def step_timing(parent_root, steps, rounds):
    base_root = parent_root or ROOT
    plain, keyed = [], []
    for r in range(rounds):
        plain.append(run_child(base_root, 0.0, steps))
        keyed.append(run_child(ROOT, CLIP_NORM, steps))
        print('round %d: %.4f ms without the key, %.4f ms with it' % (r, plain[-1]['step_ms'], keyed[-1]['step_ms']),
              file=sys.stderr, flush=True)
    p = [r['step_ms'] for r in plain]
    k = [r['step_ms'] for r in keyed]
    pm, km = float(np.median(p)), float(np.median(k))
    return {'step_without_key_from': 'the parent commit' if parent_root else 'this tree (no parent checkout given)',
            'clip_gradient_norm': CLIP_NORM, 'steps_per_run': steps, 'rounds': rounds,
            'without_key_ms': p, 'with_key_ms': k, 'without_key_median_ms': round(pm, 4),
            'with_key_median_ms': round(km, 4), 'ratio': round(km / pm, 4),
            # the margin: the spread between repetitions of the step without the key, relative to its median
            'without_key_spread': round((max(p) - min(p)) / pm, 4),
            'without_key_min_max_within_runs_ms': [min(r['min_max_ms'][0] for r in plain),
                                                   max(r['min_max_ms'][1] for r in plain)],
            'grad_stats_last_step': keyed[-1].get('grad_stats')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit, its library built')
    ap.add_argument('--no-step', action='store_true', help='the launch timings only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grad_norm.json'))
    ap.add_argument('--step-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument('--clip', type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'grad_norm_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, os.path.abspath(args.root))
    if args.step_child:
        return step_child(args.clip, args.steps)
    res = {'bench': 'grad_norm', 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'launches': launches(args.reps)}
    if not args.no_step:
        res['cfg2_step'] = step_timing(args.parent_root and os.path.abspath(args.parent_root), args.steps, args.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
