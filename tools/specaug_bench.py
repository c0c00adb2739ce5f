"""Timing of SpecAugment on the device (nabu_spec_augment_f32) next to the other input regulariser,
nabu_gaussian_noise_f32, on the same tensors ([32, 1000, 40] and [32, 1000, 123], ragged lengths), and of one cfg2
training step with the LD-style policy (W = 80, two time masks of up to 100 frames at ratio 1.0, two frequency masks of
up to 27 of 40 columns) against the plain cfg2 step.

Protocol (tools/lnlstm_bench.py): everything is warmed up, then the candidates are timed alternately, one call of each per
repetition, with device events around the call; medians are reported.

    python tools/specaug_bench.py [--reps 50] [--steps 10] [--no-step]

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nabu_amd import ops as hip, recipes                                      # noqa: E402

B, T = 32, 1000
LD = dict(time_warp=80, time_masks=2, time_mask_width=100, time_mask_ratio=1.0, freq_masks=2, freq_mask_width=27)


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernels(reps):
    rows = []
    rng = np.random.default_rng(0)
    for D, blocks in ((40, 1), (123, 3)):
        lens = rng.integers(T // 2, T + 1, B).astype(np.int32)
        lens[0] = T
        ld = torch.from_numpy(lens).cuda()
        x = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
        policies = {
            'masks': hip.SpecAugmentPolicy(**dict(LD, time_warp=0, feature_blocks=blocks)),
            'warp_masks': hip.SpecAugmentPolicy(**dict(LD, feature_blocks=blocks)),
        }
        calls = {'gaussian_noise': lambda: hip.gaussian_noise(x, 0.6, 7, 3)}
        for name, pol in policies.items():
            calls['spec_augment_' + name] = lambda pol=pol: hip.spec_augment(x, ld, pol, 7, 3)
        for _ in range(5):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                times[k].append(timed_once(fn))
        row = {'shape': [B, T, D], 'mbytes_read_plus_written': round(2 * x.numel() * 4 / 1e6, 2)}
        for k, v in times.items():
            row[k + '_us'] = round(1e3 * float(np.median(v)), 2)
            row[k + '_min_max_us'] = [round(1e3 * min(v), 2), round(1e3 * max(v), 2)]
        rows.append(row)
    return rows


def steps(n, warmup=3):
    """cfg2 (B = 32, T = 1000, 40 features, 512 units) with and without the LD policy: ms per training step"""
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    runs = {}
    for name, over in (('plain', {}), ('ld_policy', {'encoder.' + k: v for k, v in LD.items()})):
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
        data = SyntheticData(B, T, 40, min_frames=T, min_labels=20, max_labels=60, time_reduction=8, seed=4234)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                 server=None, task_index=0)
        runs[name] = (tr, [tr.to_device(data.batch(i)) for i in range(2)])
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
    out['ratio'] = round(out['ld_policy_ms_per_step'] / out['plain_ms_per_step'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='the kernel timings only')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'specaug_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'spec_augment', 'reps': args.reps, 'kernels': kernels(args.reps)}
    if not args.no_step:
        res['cfg2_step'] = dict(steps(args.steps), steps=args.steps)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
