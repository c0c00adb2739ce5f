"""Price of label smoothing in the two cross-entropy kernels: the plain entry point against the smoothing one at
smoothing = 0.1, called on the same resident buffers (logits, targets, lengths, loss, dlogits, workspace), at

  speller   [64, 100, 48]     xent_kernel: nabu_xent_loss_grad against nabu_xent_smooth_loss_grad
  dnn_wsj   [32, 1000, 3100]  wide_rows_kernel + wide_loss_sum_kernel: nabu_xent_wide_loss_grad against
                              nabu_xent_wide_smooth_loss_grad, with the GB/s of reading logits and writing dlogits once

Protocol of tools/dnn_hybrid_bench.py: warm-up calls, then device events around every call, the median over --steps
calls; the two entry points alternate call by call, so both see the same state of the machine.  Prints one JSON line
(and writes it to --out).

    python tools/xent_smooth_bench.py [--steps 50] [--warmup 5] [--out profiles/xent_smooth.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import _hip                                                     # noqa: E402
from nabu_amd.neuralnetworks.trainers import loss_functions                   # noqa: E402

SMOOTHING = 0.1
SHAPES = (('speller', (64, 100, 48), 10), ('dnn_wsj', (32, 1000, 3100), 500))        # name, [B, L, C], min length


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench(shape, min_len, steps, warmup):
    B, L, C = shape
    lib = _hip.lib()
    rng = np.random.default_rng(1)
    logits = torch.from_numpy((3 * rng.standard_normal(shape)).astype(np.float32)).cuda()
    targets = torch.from_numpy(rng.integers(0, C, (B, L)).astype(np.int32)).cuda()
    lens = rng.integers(min_len, L + 1, B).astype(np.int32)
    lens[0] = L
    ld = torch.from_numpy(lens).cuda()
    loss = torch.empty(B, device='cuda')
    dlogits = torch.empty_like(logits)
    wide = C >= loss_functions.WIDE_XENT_MIN_CLASSES
    ws_bytes = lib.nabu_xent_wide_ws_bytes(B, L) if wide else 0
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device='cuda')
    head = [B, L, C, L, _hip.ptr(logits), _hip.ptr(targets), _hip.ptr(ld), _hip.ptr(ld), 1.0 / B]
    out = [_hip.ptr(loss), _hip.ptr(dlogits)] + ([_hip.ptr(ws), ws_bytes] if wide else []) + [_hip.stream()]
    plain_fn = lib.nabu_xent_wide_loss_grad if wide else lib.nabu_xent_loss_grad
    smooth_fn = lib.nabu_xent_wide_smooth_loss_grad if wide else lib.nabu_xent_smooth_loss_grad

    def plain():
        _hip.check(plain_fn(*(head + out)), 'plain')

    def smooth():
        _hip.check(smooth_fn(*(head + [SMOOTHING] + out)), 'smooth')
    for _ in range(warmup):
        plain()
        smooth()
    torch.cuda.synchronize()
    tp, ts = [], []
    for _ in range(steps):
        tp.append(event_ms(plain))
        ts.append(event_ms(smooth))
    p, s = float(np.median(tp)), float(np.median(ts))
    res = {'shape': list(shape), 'kernel': 'wide_rows_kernel' if wide else 'xent_kernel', 'plain_ms': round(p, 4),
           'smooth_ms': round(s, 4), 'smooth_over_plain': round(s / p, 3)}
    if wide:
        gb = 2 * B * L * C * 4 / 1e9
        res.update(plain_gb_per_s=round(gb / p * 1e3, 1), smooth_gb_per_s=round(gb / s * 1e3, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'xent_smooth_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'xent_smooth', 'smoothing': SMOOTHING, 'steps': args.steps, 'device': torch.cuda.get_device_name(0)}
    for name, shape, min_len in SHAPES:
        res[name] = bench(shape, min_len, args.steps, args.warmup)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fid:
            fid.write(line + '\n')


if __name__ == '__main__':
    main()
