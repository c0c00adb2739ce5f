"""Timing of variational weight noise on the device: the noise launch alone (nabu_weight_noise_f32) over the flat
parameter buffers of cfg2 and cfg5 with the range tables the trainer builds for them, next to a device copy of the same
buffer as the yardstick, and one cfg2 and one cfg3 training step with `weight_noise = 0.075` against the plain step.

Protocol (tools/specaug_bench.py): everything is warmed up, then the candidates are timed alternately, one call of each
per repetition, with device events around the call; medians are reported.

    python tools/weight_noise_bench.py [--reps 50] [--steps 12] [--no-step] [--out profiles/weight_noise.json]

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

SIGMA = 0.075
# recipe, batch source of bench.py's leg of that name
WORKLOADS = {
    'cfg2': ('cfg2_listener_ctc', lambda: SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=60,
                                                        time_reduction=8, seed=4234)),
    'cfg3': ('cfg3_las_vanilla', lambda: SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=79,
                                                       eos=True, time_reduction=8, seed=3234)),
    'cfg5': ('cfg5_las_location', lambda: SyntheticData(64, 1600, 80, min_frames=1600, min_labels=40, max_labels=159,
                                                        eos=True, time_reduction=8, seed=5234)),
}


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def trainer(name, **over):
    recipe, source = WORKLOADS[name]
    mc, tc, ec = recipes.load_recipe(recipe, **over)
    data = source()
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0), data


def launches(reps):
    """the noise launch, the same launch with an empty table (its copy half alone) and flat_clean.copy_(flat)"""
    rows = []
    for name in ('cfg2', 'cfg5'):
        tr, _ = trainer(name, **{'trainer.weight_noise': SIGMA})
        tr._create_graph()
        tr._ensure_variables()
        tr._init_optimizer()
        flat, clean, table = tr.flat, tr.flat_clean, tr.noise_table
        kept = flat.clone()
        empty = hip.WeightNoiseTable([], flat.device)
        groups = int((table.host[:, 1] - table.host[:, 0]).sum())
        calls = {'weight_noise': lambda: hip.weight_noise(flat, clean, table, SIGMA, 7, 3),
                 'weight_noise_empty_table': lambda: hip.weight_noise(flat, clean, empty, SIGMA, 7, 3),
                 'device_copy': lambda: clean.copy_(flat)}
        for _ in range(5):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                times[k].append(timed_once(fn))
        flat.copy_(kept)
        n = flat.numel()
        row = {'workload': name, 'flat_elements': n, 'ranges': table.n, 'noisy_elements': 4 * groups,
               'mbytes_copy': round(2 * n * 4 / 1e6, 2), 'mbytes_noise': round((2 * n + 4 * groups) * 4 / 1e6, 2)}
        for k, v in times.items():
            row[k + '_us'] = round(1e3 * float(np.median(v)), 2)
            row[k + '_min_max_us'] = [round(1e3 * min(v), 2), round(1e3 * max(v), 2)]
        row['noise_over_copy'] = round(row['weight_noise_us'] / row['device_copy_us'], 3)
        row['noise_gb_per_s'] = round(row['mbytes_noise'] / row['weight_noise_us'] * 1e3, 1)
        row['copy_gb_per_s'] = round(row['mbytes_copy'] / row['device_copy_us'] * 1e3, 1)
        row['noisy_gelements_per_s'] = round(4 * groups / row['weight_noise_us'] / 1e3, 2)
        rows.append(row)
        del tr, flat, clean, kept
        torch.cuda.empty_cache()
    return rows


def steps(name, n, warmup=3):
    """Trainer.step on resident batches with and without the key, alternating: ms per training step"""
    runs = {}
    for key, over in (('plain', {}), ('weight_noise', {'trainer.weight_noise': SIGMA})):
        tr, data = trainer(name, **over)
        runs[key] = (tr, [tr.to_device(data.batch(i)) for i in range(2)])
    for i in range(warmup):
        for tr, batches in runs.values():
            tr.step(batches[i % 2])
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for i in range(n):
        for k, (tr, batches) in runs.items():
            times[k].append(timed_once(lambda: tr.step(batches[i % 2])))
    out = {k + '_ms_per_step': round(float(np.median(v)), 3) for k, v in times.items()}
    out.update({k + '_min_max_ms': [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
    out['ratio'] = round(out['weight_noise_ms_per_step'] / out['plain_ms_per_step'], 4)
    out['steps'] = n
    del runs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--no-step', action='store_true', help='the launch timings only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_noise.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'weight_noise_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'weight_noise', 'stddev': SIGMA, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
           'launches': launches(args.reps)}
    if not args.no_step:
        for name in ('cfg2', 'cfg3'):
            res[name + '_step'] = steps(name, args.steps)
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
