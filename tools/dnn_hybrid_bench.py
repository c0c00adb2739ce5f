"""Timing of the Kaldi-hybrid recipe (config/recipes/dnn_hybrid_wsj) at full size on synthetic data: B = 32
utterances of up to T = 1000 frames (min_frames = 500), 123 features, 3100 HMM states.

Prints one JSON line per measurement:
  step        median ms per training step (device events around each of --steps steps after --warmup), frames/s
              (valid frames), whole-step FLOP/s from the shapes (forward + backward of every dense product, less the
              first layer's input gradient);
  xent        xent_kernel (nabu_xent_loss_grad) against nabu_xent_wide_loss_grad on the same [32, 1000, 3100]
              logits;
  relu_ln     the fused relu + per-row layer norm (nabu_rows_relu_ln_fwd / _bwd) against relu + layer_norm_fwd /
              layer_norm_bwd (+ relu_bwd) on [N, 2048].

    python tools/dnn_hybrid_bench.py [--steps 20] [--warmup 3] [--precision bf16x6] [--only step|xent|relu_ln]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import ops as hip                                               # noqa: E402
from nabu_amd import recipes                                                  # noqa: E402
from nabu_amd.neuralnetworks.models.ed_encoders import dnn as dnn_enc         # noqa: E402
from nabu_amd.neuralnetworks.trainers import trainer_factory                  # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402

B, T, F, C, MIN_FRAMES = 32, 1000, 123, 3100, 500


def timed(fn, reps, warmup=2):
    """median milliseconds of fn() over reps device-event pairs"""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def step_flops(lens, Tm, context, units, layers):
    """dense-product FLOP of one step: first layer forward + weight gradient (no input gradient), every other
    hidden layer forward + input gradient + weight gradient, the output layer the same on all B x Tm frames"""
    N = float(np.sum(lens))
    K = (2 * context - 1) * F
    return 2 * 2 * N * K * units + (layers - 1) * 3 * 2 * N * units * units + 3 * 2 * B * Tm * units * C


def bench_step(args):
    over = {'trainer.batch_size': B}
    if args.precision:
        over['encoder.gemm_precision'] = args.precision
    mc, tc, ec = recipes.load_recipe('dnn_hybrid_wsj', **over)
    data = SyntheticData(B, T, F, num_labels=C, min_frames=MIN_FRAMES, frame_targets=True, target_name='alignments',
                         seed=11)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=None, task_index=0)
    raw = data.batch(0)
    batch = tr.to_device(raw)
    for _ in range(args.warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    ms = timed(lambda: tr.step(batch), args.steps, warmup=0)
    lens = raw['input_seq_length']['features']
    enc = tr.model.encoder.conf
    flops = step_flops(lens, int(lens.max()), int(enc['context']), int(enc['num_units']), int(enc['num_layers']))
    print(json.dumps({'bench': 'dnn_hybrid_step', 'precision': enc['gemm_precision'], 'B': B, 'T': T,
                      'frames': int(lens.sum()), 'ms_per_step': round(ms, 3),
                      'frames_per_s': round(float(lens.sum()) / ms * 1e3, 1),
                      'step_tflop': round(flops / 1e12, 3), 'tflop_per_s': round(flops / ms / 1e9, 1)}), flush=True)


def bench_xent(args):
    rng = np.random.default_rng(1)
    logits = torch.from_numpy((3 * rng.standard_normal((B, T, C))).astype(np.float32)).cuda()
    lens = np.random.default_rng(2).integers(MIN_FRAMES, T + 1, B).astype(np.int32)
    lens[0] = T
    targets = torch.from_numpy(rng.integers(0, C, (B, T)).astype(np.int32)).cuda()
    ld = torch.from_numpy(lens).cuda()
    old = timed(lambda: hip.xent_loss_grad(logits, targets, ld, ld, 1.0 / B), max(3, args.steps // 4))
    new = timed(lambda: hip.xent_wide_loss_grad(logits, targets, ld, ld, 1.0 / B), args.steps)
    gb = 2 * B * T * C * 4 / 1e9
    print(json.dumps({'bench': 'xent', 'shape': [B, T, C], 'xent_kernel_ms': round(old, 3),
                      'xent_wide_ms': round(new, 3), 'wide_gb_per_s': round(gb / new * 1e3, 1)}), flush=True)


def bench_relu_ln(args):
    rng = np.random.default_rng(3)
    lens = np.random.default_rng(2).integers(MIN_FRAMES, T + 1, B)
    lens[0] = T
    N, H = int(lens.sum()), 2048
    z = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.standard_normal((N, H)).astype(np.float32)).cuda()
    g = torch.ones(H, device='cuda')
    b = torch.zeros(H, device='cuda')
    dg = torch.zeros(H, device='cuda')
    db = torch.zeros(H, device='cuda')
    y, mean, rstd = hip.rows_relu_ln_fwd(z, g, b)

    def fused_bwd():
        dz, dgp, dbp = hip.rows_relu_ln_bwd(z, dy, g, mean, rstd)
        hip.colsum(dgp, dg)
        hip.colsum(dbp, db)
    r = hip.relu(z)
    y2, m2, s2 = hip.layer_norm_fwd(r, g, b)

    def split_fwd():
        r_ = hip.relu(z)
        hip.layer_norm_fwd(r_, g, b)

    def split_bwd():
        dr, dgp, dbp = hip.layer_norm_bwd(r, g, dy, m2, s2)
        hip.colsum(dgp, dg)
        hip.colsum(dbp, db)
        hip.relu_bwd(r, dr)
    res = {'bench': 'relu_ln', 'shape': [N, H],
           'fused_fwd_ms': timed(lambda: hip.rows_relu_ln_fwd(z, g, b), args.steps),
           'fused_bwd_ms': timed(fused_bwd, args.steps),
           'split_fwd_ms': timed(split_fwd, args.steps),
           'split_bwd_ms': timed(split_bwd, args.steps)}
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default=None, help='encoder gemm_precision (default: the recipe\'s)')
    ap.add_argument('--only', choices=('step', 'xent', 'relu_ln'), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'dnn_hybrid_bench needs a GPU'
    torch.cuda.set_device(0)
    for name, fn in (('xent', bench_xent), ('relu_ln', bench_relu_ln), ('step', bench_step)):
        if args.only in (None, name):
            fn(args)
    assert dnn_enc.splice_ld(F, 5) == 1120


if __name__ == '__main__':
    main()
