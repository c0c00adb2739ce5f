"""The convolution-module kernels (conv_module.hip) against the best alternative a user of this stack has today, at B 32,
D 256, lengths T/2 .. T, T 250 (the conformer_ctc recipe behind its front end) and T 1000 (without it), K 15 and 31:

  forward   nabu_conv_module_fwd (one launch) against the unfused composition in torch fp32 on the same operands:
            F.glu, the padding mask on its result, F.conv1d(groups=D), F.layer_norm, F.silu
  backward  nabu_conv_module_bwd (two launches and the two colsum calls: the whole call) against torch.autograd.grad of
            that composition (graph retained, backward only)
  bytes     what the algorithm must move — u read and y written forward; u and dy read and du written backward, from
            the shapes — over the measured time, next to a device copy that moves the same number of bytes in the same
            rotation
  step      one training step of conformer_ctc with feature_blocks = 3 at cfg1's size (8 x 200 x 123) against
            transformer_ctc on the same batches — for information, no bar

The bar, forward and backward: no slower than torch.  Protocol of the other tools (tools/self_attn_bench.py): warm-up,
medians of --rounds rounds of --calls calls between device events, all sides alternating round by round in the same
run; the spread of the round times is reported with them.  Prints one JSON line (and writes it to --out).

    python tools/conformer_conv_bench.py [--rounds 5] [--calls 200] [--out profiles/conformer_conv.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import ops as hip, recipes                                      # noqa: E402
from nabu_amd.neuralnetworks.components import layer                          # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402
from tools.conv_frontend_bench import rounds_ms                               # noqa: E402

B, D = 32, 256


def module_bench(T, K, rounds, calls):
    g = torch.Generator(device='cuda').manual_seed(1)
    u = torch.randn((B, T, 2 * D), device='cuda', generator=g).requires_grad_()
    dy = torch.randn((B, T, D), device='cuda', generator=g)
    w = (torch.randn((K, D), device='cuda', generator=g) / K ** 0.5).requires_grad_()
    bw, beta = (0.1 * torch.randn(D, device='cuda', generator=g) for _ in range(2))
    gamma = 1 + 0.1 * torch.randn(D, device='cuda', generator=g)
    bw, gamma, beta = (t.requires_grad_() for t in (bw, gamma, beta))
    host_lens = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    host_lens[0] = T
    lens = torch.from_numpy(host_lens).cuda()
    valid = (torch.arange(T, device='cuda')[None, :] < lens[:, None])[:, :, None].float()       # [B,T,1]
    wt = w.t()[:, None, :]

    def torch_fwd():
        gl = (F.glu(u, dim=2) * valid).transpose(1, 2)
        z = F.conv1d(gl, wt, bw, padding=(K - 1) // 2, groups=D).transpose(1, 2)
        return F.silu(F.layer_norm(z, (D,), gamma, beta, layer.LN_EPS))
    ref, dy_ref = torch_fwd(), dy * valid                                     # (no gradient enters a padding row)
    leaves = (u, w, bw, gamma, beta)
    ud, par = u.detach(), [t.detach() for t in (w, bw, gamma, beta)]
    y, mean, rstd = hip.conv_module_fwd(ud, lens, *par, layer.LN_EPS)
    got = hip.conv_module_bwd(ud, lens, *par, mean, rstd, dy)
    want = torch.autograd.grad(ref, leaves, dy_ref, retain_graph=True)
    worst_fwd = float((ref.detach() * valid - y).abs().max())
    worst_bwd = max(float((a - b).abs().max() / b.abs().max()) for a, b in
                    zip(got, (want[0] * valid, want[1], want[2], want[3], want[4])))
    fwd_bytes, bwd_bytes = 4 * B * T * 3 * D, 4 * B * T * 5 * D
    src = [torch.empty(n // 8, dtype=torch.float32, device='cuda').normal_() for n in (fwd_bytes, bwd_bytes)]
    dst = [torch.empty_like(s) for s in src]                                  # a copy reads n/2 bytes and writes n/2
    (f, fs), (rf, rfs), (bw_, bs), (rb, rbs), (cf, _), (cb, _) = rounds_ms(
        [lambda: hip.conv_module_fwd(ud, lens, *par, layer.LN_EPS), torch_fwd,
         lambda: hip.conv_module_bwd(ud, lens, *par, mean, rstd, dy),
         lambda: torch.autograd.grad(ref, leaves, dy_ref, retain_graph=True),
         lambda: dst[0].copy_(src[0]), lambda: dst[1].copy_(src[1])], rounds, calls)

    def r(x):
        return round(x, 4)
    return {'shape': [B, T, D, K], 'fwd_ms': r(f), 'fwd_spread': [r(x) for x in fs], 'torch_fwd_ms': r(rf),
            'torch_fwd_spread': [r(x) for x in rfs], 'fwd_over_torch': round(f / rf, 3), 'fwd_bar': 'met' if f <= rf else 'missed',
            'fwd_gbytes_per_s': round(fwd_bytes / f / 1e6, 1), 'copy_fwd_gbytes_per_s': round(fwd_bytes / cf / 1e6, 1),
            'bwd_ms': r(bw_), 'bwd_spread': [r(x) for x in bs], 'torch_bwd_ms': r(rb), 'torch_bwd_spread': [r(x) for x in rbs],
            'bwd_over_torch': round(bw_ / rb, 3), 'bwd_bar': 'met' if bw_ <= rb else 'missed',
            'bwd_gbytes_per_s': round(bwd_bytes / bw_ / 1e6, 1), 'copy_bwd_gbytes_per_s': round(bwd_bytes / cb / 1e6, 1),
            'max_abs_diff_fwd': worst_fwd, 'max_rel_diff_bwd': worst_bwd}


def step_bench(rounds, calls):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    data = SyntheticData(8, 200, 123, min_frames=120, min_labels=5, max_labels=20, time_reduction=4, seed=2234)
    trainers = []
    for recipe in ('conformer_ctc', 'transformer_ctc'):
        mc, tc, ec = recipes.load_recipe(recipe, **{'encoder.feature_blocks': 3})
        trainers.append(trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                                            expdir=None, server=None, task_index=0))
    batches = [[tr.to_device(data.batch(i)) for i in range(4)] for tr in trainers]
    count = [0, 0]

    def stepper(k):
        def fn():
            trainers[k].step(batches[k][count[k] % 4])
            count[k] += 1
        return fn
    (cf, cs), (tf, ts) = rounds_ms([stepper(0), stepper(1)], rounds, calls)
    return {'shape': [8, 200, 123], 'conformer_ctc_step_ms': round(cf, 3), 'conformer_spread': [round(v, 3) for v in cs],
            'transformer_ctc_step_ms': round(tf, 3), 'transformer_spread': [round(v, 3) for v in ts],
            'conformer_over_transformer': round(cf / tf, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conformer_conv_bench needs a GPU'
    torch.cuda.set_device(0)
    res = {'bench': 'conformer_conv', 'rounds': args.rounds, 'calls': args.calls, 'device': torch.cuda.get_device_name(0),
           'module': [module_bench(T, K, args.rounds, args.calls) for T in (250, 1000) for K in (15, 31)],
           'step': step_bench(args.rounds, args.calls)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fid:
            fid.write(line + '\n')


if __name__ == '__main__':
    main()
