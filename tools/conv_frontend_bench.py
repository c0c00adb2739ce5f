"""The convolutional front end (conv2d.hip) against its yardsticks, at B 32, T 1000, F 41 for the layers of
`conv_channels = 64 128`:

  forward   nabu_conv3x3_relu_fwd against nabu_gemm_f32 on the same layer's MATERIALISED im2col product
            [B T F, 9 Cin] x [9 Cin, Cout] (the im2col matrix is built beforehand and not timed).  The bar: no slower —
            the matrix work is identical and the convolution reads about a ninth of the operand bytes.  The first layer
            (K = 27) is reported without a bar.
  wgrad     nabu_conv3x3_bwd_weights (both launches) against the forward launch of the same layer
  step      one training step of the vgg_dblstm_ctc recipe with feature_blocks = 3 at cfg1's size (8 x 200 x 123) against
            plain cfg1 on the same batches

Protocol of the other tools: warm-up, then medians of --rounds rounds of --calls calls between device events, the two
sides of a comparison alternating round by round in the same run; the spread of the round times is reported with them.
Prints one JSON line (and writes it to --out).

    python tools/conv_frontend_bench.py [--rounds 5] [--calls 200] [--out profiles/conv_frontend.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import ops as hip, recipes                                      # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402

B, T, F = 32, 1000, 41
LAYERS = (('block0/conv0', T, F, 3, 64), ('block0/conv1', T, F, 64, 64),
          ('block1/conv0', T // 2, (F + 1) // 2, 64, 128), ('block1/conv1', T // 2, (F + 1) // 2, 128, 128))


def rounds_ms(fns, rounds, calls):
    """per-call milliseconds of each fn: [median over rounds, (min, max)], the fns alternating round by round"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return [(float(np.median(t)), (float(min(t)), float(max(t)))) for t in times]


def im2col(x):
    """[B,T,F,C] -> [B T F, 9 C], taps in (kt, kf) order, zero "same" padding (full-length utterances)"""
    Bn, Tn, Fn, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = torch.stack([xp[:, kt:kt + Tn, kf:kf + Fn] for kt in range(3) for kf in range(3)], dim=3)
    return cols.reshape(Bn * Tn * Fn, 9 * C).contiguous()


def layer_bench(name, Tn, Fn, Cin, Cout, rounds, calls):
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn((B, Tn, Fn, Cin), device='cuda', generator=g)
    w = torch.randn((3, 3, Cin, Cout), device='cuda', generator=g) * 0.05
    bias = torch.zeros(Cout, device='cuda')
    lens = torch.full((B,), Tn, dtype=torch.int32, device='cuda')
    cols = im2col(x)
    w2 = w.reshape(9 * Cin, Cout)
    c = torch.empty((cols.shape[0], Cout), device='cuda')
    y = hip.conv3x3_relu(x, lens, w, bias)
    hip.gemm(cols, w2, c, bias=bias)
    worst = float((torch.relu(c).view_as(y) - y).abs().max())          # the two sides compute the same layer
    dy = torch.randn(y.shape, device='cuda', generator=g)
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    (conv, cs), (gemm, gs), (wg, ws) = rounds_ms(
        [lambda: hip.conv3x3_relu(x, lens, w, bias), lambda: hip.gemm(cols, w2, c, bias=bias),
         lambda: hip.conv3x3_bwd_weights(x, dy, y, lens, dw, db)], rounds, calls)
    flops = 2.0 * cols.shape[0] * 9 * Cin * Cout
    return {'layer': name, 'shape': [B, Tn, Fn, Cin, Cout], 'conv_ms': round(conv, 4), 'conv_spread': [round(v, 4) for v in cs],
            'gemm_im2col_ms': round(gemm, 4), 'gemm_spread': [round(v, 4) for v in gs],
            'conv_over_gemm': round(conv / gemm, 3), 'bar': 'none (K = 27)' if Cin < 4 else 'met' if conv <= gemm else 'missed',
            'conv_tflops': round(flops / conv / 1e9, 1), 'wgrad_ms': round(wg, 4), 'wgrad_spread': [round(v, 4) for v in ws],
            'wgrad_over_conv': round(wg / conv, 3), 'max_abs_diff_to_gemm': worst}


def step_bench(rounds, calls):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    data = SyntheticData(8, 200, 123, min_frames=120, min_labels=5, max_labels=20, time_reduction=4, seed=2234)
    trainers = []
    for recipe, over in (('vgg_dblstm_ctc', {'encoder.feature_blocks': 3}), ('cfg1_dblstm_ctc', {})):
        mc, tc, ec = recipes.load_recipe(recipe, **over)
        trainers.append(trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                                            expdir=None, server=None, task_index=0))
    batches = [[tr.to_device(data.batch(i)) for i in range(4)] for tr in trainers]
    count = [0, 0]

    def stepper(k):
        def fn():
            trainers[k].step(batches[k][count[k] % 4])
            count[k] += 1
        return fn
    (vgg, vs_), (plain, ps) = rounds_ms([stepper(0), stepper(1)], rounds, calls)
    return {'shape': [8, 200, 123], 'vgg_dblstm_step_ms': round(vgg, 3), 'vgg_spread': [round(v, 3) for v in vs_],
            'cfg1_step_ms': round(plain, 3), 'cfg1_spread': [round(v, 3) for v in ps], 'vgg_over_cfg1': round(vgg / plain, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_frontend_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'conv_frontend', 'rounds': args.rounds, 'calls': args.calls, 'device': torch.cuda.get_device_name(0),
           'layers': [layer_bench(*layer, rounds=args.rounds, calls=args.calls) for layer in LAYERS],
           'step': step_bench(args.rounds, args.calls)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fid:
            fid.write(line + '\n')


if __name__ == '__main__':
    main()
