"""The self-attention kernels (self_attn.hip) against the best alternative a user of this stack has today, at B 32, H 4,
dk 64 and T 250 (the transformer_ctc recipe behind its front end) and T 1000 (without it):

  forward   nabu_self_attn_fwd against torch.nn.functional.scaled_dot_product_attention in fp32 on the same operands
            (given as contiguous [B,H,T,dk] tensors), the padding expressed as its boolean key mask
  backward  nabu_self_attn_bwd (both launches) against torch.autograd.grad of that call (graph retained, backward only)
  step      one training step of the transformer_ctc recipe with feature_blocks = 3 at cfg1's size (8 x 200 x 123) against
            vgg_dblstm_ctc on the same batches — for information, no bar

  --bf16    instead of all of the above: nabu_self_attn_bf16_fwd / _bwd (self_attn_bf16.hip) against the fp32 kernels on the
            same operands, and against scaled_dot_product_attention on bf16 tensors (its conversions not timed,
            torch.autograd.grad as its backward side), the three sides alternating in one run.  The bar: no slower than
            the fp32 kernels; the ratio against bf16 SDPA is for information

  --dropout instead of all of the above: the kernels with dropout on the attention probabilities (keep 0.9), fp32 and
            bf16, forward and whole backward call, against the plain kernels on the same operands and ONE nabu_dropout_f32
            launch over B H T T floats.  The bars: forward no slower than plain + one such pass, backward no slower
            than plain + two (the mask alone costs an unfused implementation at least that).  With --parent-lib, the
            plain kernels of a library built from the parent commit run beside this build's: the ratio must lie inside
            the spread

  --window  instead of all of the above: the chunk-window kernels (nabu_self_attn[_bf16]_win_*), fp32 and bf16, forward
            and whole backward call, at (chunk, left_chunks) = (1, -1), (16, -1), (16, 4) and (T, -1), against the plain
            kernels on the same operands; (T, -1) walks every tile and shows what the predicate alone costs.  The bar:
            every truly windowed side no slower than the plain kernel.  Reported beside each ratio: the fraction of
            tiles walked; for information, fp32 scaled_dot_product_attention forward with the same boolean mask.
            --parent-lib as with --dropout

The bar, forward and backward: no slower.  Lengths are drawn uniformly from T/2 .. T (one row at T).
Protocol of the other tools: warm-up, then medians of --rounds rounds of --calls calls between device events, the two
sides of a comparison alternating round by round in the same run; the spread of the round times is reported with them.
Prints one JSON line (and writes it to --out).

    python tools/self_attn_bench.py [--rounds 5] [--calls 200] [--out profiles/self_attn.json]
    python tools/self_attn_bench.py --bf16 --out profiles/self_attn_bf16.json
    python tools/self_attn_bench.py --dropout [--parent-lib PATH] --out profiles/self_attn_dropout.json
    python tools/self_attn_bench.py --window [--parent-lib PATH] --out profiles/self_attn_window.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import ops as hip, recipes                                      # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402
from tools.conv_frontend_bench import rounds_ms                               # noqa: E402

B, H, DK = 32, 4, 64


def attn_bench(T, rounds, calls):
    D = H * DK
    g = torch.Generator(device='cuda').manual_seed(1)
    qkv = torch.randn((B, T, 3 * D), device='cuda', generator=g)
    do = torch.randn((B, T, D), device='cuda', generator=g)
    host_lens = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    host_lens[0] = T
    lens = torch.from_numpy(host_lens).cuda()
    q, k, v = (t.contiguous().requires_grad_() for t in qkv.view(B, T, 3, H, DK).permute(2, 0, 3, 1, 4))
    valid = torch.arange(T, device='cuda')[None, :] < lens[:, None]          # [B,T]
    mask = valid[:, None, None, :]
    sdpa = torch.nn.functional.scaled_dot_product_attention
    ref = sdpa(q, k, v, attn_mask=mask)
    do_ref = (do * valid[:, :, None]).view(B, T, H, DK).transpose(1, 2).contiguous()       # (no gradient enters a padding row)
    o, lse = hip.self_attn_fwd(qkv, lens, H)
    dqkv = hip.self_attn_bwd(qkv, o, lse, do, lens, H)
    grads = torch.autograd.grad(ref, (q, k, v), do_ref, retain_graph=True)
    want = ref.detach().transpose(1, 2).reshape(B, T, D) * valid[:, :, None]
    worst_fwd = float((want - o).abs().max())
    want = torch.stack([t.transpose(1, 2).reshape(B, T, D) for t in grads], dim=2).reshape(B, T, 3 * D)
    worst_bwd = float((want - dqkv).abs().max())
    (f, fs), (rf, rfs), (bw, bs), (rb, rbs) = rounds_ms(
        [lambda: hip.self_attn_fwd(qkv, lens, H), lambda: sdpa(q, k, v, attn_mask=mask),
         lambda: hip.self_attn_bwd(qkv, o, lse, do, lens, H),
         lambda: torch.autograd.grad(ref, (q, k, v), do_ref, retain_graph=True)], rounds, calls)
    pairs = float((host_lens.astype(np.float64) ** 2).sum()) * H

    def r(x):
        return round(x, 4)
    return {'shape': [B, T, H, DK], 'fwd_ms': r(f), 'fwd_spread': [r(x) for x in fs], 'sdpa_fwd_ms': r(rf),
            'sdpa_fwd_spread': [r(x) for x in rfs], 'fwd_over_sdpa': round(f / rf, 3), 'fwd_bar': 'met' if f <= rf else 'missed',
            'fwd_tflops': round(4 * pairs * DK / f / 1e9, 1), 'bwd_ms': r(bw), 'bwd_spread': [r(x) for x in bs],
            'sdpa_bwd_ms': r(rb), 'sdpa_bwd_spread': [r(x) for x in rbs], 'bwd_over_sdpa': round(bw / rb, 3),
            'bwd_bar': 'met' if bw <= rb else 'missed', 'bwd_tflops_useful': round(10 * pairs * DK / bw / 1e9, 1),
            'max_abs_diff_fwd': worst_fwd, 'max_abs_diff_bwd': worst_bwd}


def attn_bf16_bench(T, rounds, calls):
    """the bf16 kernels, the fp32 kernels and bf16 SDPA on the operands of attn_bench, alternating in one run"""
    D = H * DK
    g = torch.Generator(device='cuda').manual_seed(1)
    qkv = torch.randn((B, T, 3 * D), device='cuda', generator=g)
    do = torch.randn((B, T, D), device='cuda', generator=g)
    host_lens = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    host_lens[0] = T
    lens = torch.from_numpy(host_lens).cuda()
    q, k, v = (t.contiguous().bfloat16().requires_grad_() for t in qkv.view(B, T, 3, H, DK).permute(2, 0, 3, 1, 4))
    valid = torch.arange(T, device='cuda')[None, :] < lens[:, None]
    mask = valid[:, None, None, :]
    sdpa = torch.nn.functional.scaled_dot_product_attention
    ref = sdpa(q, k, v, attn_mask=mask)
    do_ref = (do * valid[:, :, None]).view(B, T, H, DK).transpose(1, 2).contiguous().bfloat16()
    o, lse = hip.self_attn_fwd(qkv, lens, H)
    o16, lse16 = hip.self_attn_fwd(qkv, lens, H, 'bf16')
    dqkv = hip.self_attn_bwd(qkv, o, lse, do, lens, H)
    dqkv16 = hip.self_attn_bwd(qkv, o16, lse16, do, lens, H, 'bf16')
    sides = rounds_ms(
        [lambda: hip.self_attn_fwd(qkv, lens, H, 'bf16'), lambda: hip.self_attn_fwd(qkv, lens, H),
         lambda: sdpa(q, k, v, attn_mask=mask),
         lambda: hip.self_attn_bwd(qkv, o16, lse16, do, lens, H, 'bf16'), lambda: hip.self_attn_bwd(qkv, o, lse, do, lens, H),
         lambda: torch.autograd.grad(ref, (q, k, v), do_ref, retain_graph=True)], rounds, calls)
    pairs = float((host_lens.astype(np.float64) ** 2).sum()) * H
    res = {'shape': [B, T, H, DK], 'max_abs_diff_fwd_bf16_f32': float((o16 - o).abs().max()),
           'max_abs_diff_bwd_bf16_f32': float((dqkv16 - dqkv).abs().max())}
    for name, (ms, spread) in zip(('fwd_bf16', 'fwd_f32', 'sdpa_bf16_fwd', 'bwd_bf16', 'bwd_f32', 'sdpa_bf16_bwd'), sides):
        res[name + '_ms'], res[name + '_spread'] = round(ms, 4), [round(x, 4) for x in spread]
    for d, flops in (('fwd', 4), ('bwd', 10)):
        new, f32, ref_ms = res[d + '_bf16_ms'], res[d + '_f32_ms'], res['sdpa_bf16_%s_ms' % d]
        res[d + '_bf16_over_f32'], res[d + '_bar'] = round(new / f32, 3), 'met' if new <= f32 else 'missed'
        res[d + '_bf16_over_sdpa_bf16'] = round(new / ref_ms, 3)
        res[d + '_bf16_tflops' + ('_useful' if d == 'bwd' else '')] = round(flops * pairs * DK / new / 1e9, 1)
    return res


def attn_dropout_bench(T, rounds, calls, parent):
    """the dropout kernels (keep 0.9) of both precisions, the plain kernels on the same operands and one nabu_dropout_f32
    pass over B H T T floats (what the mask alone costs an unfused implementation, once forward and twice backward),
    alternating in one run; with `parent` (a libnabu_hip.so built from the parent commit) its plain kernels too"""
    D, keep, rng = H * DK, 0.9, (1234, 5)
    g = torch.Generator(device='cuda').manual_seed(1)
    qkv = torch.randn((B, T, 3 * D), device='cuda', generator=g)
    do = torch.randn((B, T, D), device='cuda', generator=g)
    host_lens = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    host_lens[0] = T
    lens = torch.from_numpy(host_lens).cuda()
    probs = torch.rand((B * H * T * T,), device='cuda', generator=g)
    names, fns, kept = [], [], {}
    for p in ('f32', 'bf16'):
        for tag, kw in (('drop', dict(keep=keep, rng=rng)), ('plain', {})):
            o, lse = kept[p, tag] = hip.self_attn_fwd(qkv, lens, H, p, **kw)
            names += ['fwd_%s_%s' % (tag, p), 'bwd_%s_%s' % (tag, p)]
            fns += [lambda p=p, kw=kw: hip.self_attn_fwd(qkv, lens, H, p, **kw),
                    lambda p=p, kw=kw, o=o, lse=lse: hip.self_attn_bwd(qkv, o, lse, do, lens, H, p, **kw)]
    names.append('dropout_pass')
    fns.append(lambda: hip.dropout(probs, keep, *rng))
    if parent is not None:
        from nabu_amd import _hip
        out_o, out_lse, out_d = torch.empty_like(do), torch.empty((B, H, T), device='cuda'), torch.empty_like(qkv)
        for p, stem in (('f32', 'nabu_self_attn'), ('bf16', 'nabu_self_attn_bf16')):
            o, lse = kept[p, 'plain']
            names += ['fwd_parent_%s' % p, 'bwd_parent_%s' % p]
            fns += [lambda f=getattr(parent, stem + '_fwd'): f(B, T, H, DK, qkv.data_ptr(), 3 * D, lens.data_ptr(), out_o.data_ptr(),
                                                                out_lse.data_ptr(), _hip.stream()),
                    lambda f=getattr(parent, stem + '_bwd'), o=o, lse=lse: f(B, T, H, DK, qkv.data_ptr(), 3 * D, o.data_ptr(), lse.data_ptr(),
                                                                             do.data_ptr(), lens.data_ptr(), out_d.data_ptr(), _hip.stream())]
    res = {'shape': [B, T, H, DK], 'keep': keep}
    for name, (ms, spread) in zip(names, rounds_ms(fns, rounds, calls)):
        res[name + '_ms'], res[name + '_spread'] = round(ms, 4), [round(x, 4) for x in spread]
    for p in ('f32', 'bf16'):
        for d, passes in (('fwd', 1), ('bwd', 2)):
            new, bar = res['%s_drop_%s_ms' % (d, p)], res['%s_plain_%s_ms' % (d, p)] + passes * res['dropout_pass_ms']
            res['%s_%s_drop_over_plain' % (d, p)] = round(new / res['%s_plain_%s_ms' % (d, p)], 3)
            res['%s_%s_bar_ms' % (d, p)], res['%s_%s_bar' % (d, p)] = round(bar, 4), 'met' if new <= bar else 'missed'
            if parent is not None:
                res['%s_%s_plain_over_parent' % (d, p)] = round(res['%s_plain_%s_ms' % (d, p)] / res['%s_parent_%s_ms' % (d, p)], 4)
    return res


def tiles_walked(lens, T, TQ, TK, window):
    """(key tiles the forward and dQ workgroups walk, query tiles the dK/dV workgroups walk) over the batch, by the rule
    of csrc/attn_win.h; window None: every tile below len"""
    fwd = dkv = 0
    for L in (int(x) for x in lens):
        if window is not None:
            C = min(window[0], max(T, 1))
            Lc = -1 if window[1] >= (max(T, 1) - 1) // C else window[1]
        for r0 in range(0, L, TQ):
            last = min(r0 + TQ, L) - 1
            if window is None:
                fwd, dkv = fwd + -(-L // TK), dkv + -(-L // TK)
                continue
            lo = 0 if Lc < 0 else max(0, r0 // C * C - Lc * C)
            fwd += -(-min(L, (last // C + 1) * C) // TK) - lo // TK
            dkv += -(-(L if Lc < 0 else min(L, (last // C + Lc + 1) * C)) // TK) - (r0 // C * C) // TK
    return fwd, dkv


def attn_window_bench(T, rounds, calls, parent):
    """the windowed kernels of both precisions at (C, Lc) = (1, -1), (16, -1), (16, 4) and (T, -1) — the last walks every
    tile and shows what the predicate alone costs — and the plain kernels on the same operands, alternating in one run; for
    information fp32 scaled_dot_product_attention forward with the same boolean masks; with `parent` (a libnabu_hip.so
    built from the parent commit) its plain kernels too.  Each ratio stands beside the fraction of tiles walked."""
    D = H * DK
    g = torch.Generator(device='cuda').manual_seed(1)
    qkv = torch.randn((B, T, 3 * D), device='cuda', generator=g)
    do = torch.randn((B, T, D), device='cuda', generator=g)
    host_lens = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    host_lens[0] = T
    lens = torch.from_numpy(host_lens).cuda()
    windows = {'plain': None, 'c1': (1, -1), 'c16': (16, -1), 'c16_l4': (16, 4), 'cT': (T, -1)}
    names, fns, kept = [], [], {}
    for p in ('f32', 'bf16'):
        for tag, win in windows.items():
            o, lse = kept[p, tag] = hip.self_attn_fwd(qkv, lens, H, p, window=win)
            names += ['fwd_%s_%s' % (tag, p), 'bwd_%s_%s' % (tag, p)]
            fns += [lambda p=p, win=win: hip.self_attn_fwd(qkv, lens, H, p, window=win),
                    lambda p=p, win=win, o=o, lse=lse: hip.self_attn_bwd(qkv, o, lse, do, lens, H, p, window=win)]
    q, k, v = (t.contiguous() for t in qkv.view(B, T, 3, H, DK).permute(2, 0, 3, 1, 4))
    i, j = torch.arange(T, device='cuda')[None, :, None], torch.arange(T, device='cuda')[None, None, :]
    for tag in ('c1', 'c16', 'c16_l4'):
        C, Lc = windows[tag]
        hi = torch.minimum(lens[:, None, None], (i // C + 1) * C)
        mask = ((j < hi) & (j >= (0 if Lc < 0 else (i // C - Lc) * C)) | (i == j))[:, None]      # (a padding row sees itself: no NaN)
        names.append('sdpa_fwd_%s_f32' % tag)
        fns.append(lambda mask=mask: torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask))
    if parent is not None:
        from nabu_amd import _hip
        out_o, out_lse, out_d = torch.empty_like(do), torch.empty((B, H, T), device='cuda'), torch.empty_like(qkv)
        for p, stem in (('f32', 'nabu_self_attn'), ('bf16', 'nabu_self_attn_bf16')):
            o, lse = kept[p, 'plain']
            names += ['fwd_parent_%s' % p, 'bwd_parent_%s' % p]
            fns += [lambda f=getattr(parent, stem + '_fwd'): f(B, T, H, DK, qkv.data_ptr(), 3 * D, lens.data_ptr(), out_o.data_ptr(),
                                                                out_lse.data_ptr(), _hip.stream()),
                    lambda f=getattr(parent, stem + '_bwd'), o=o, lse=lse: f(B, T, H, DK, qkv.data_ptr(), 3 * D, o.data_ptr(), lse.data_ptr(),
                                                                             do.data_ptr(), lens.data_ptr(), out_d.data_ptr(), _hip.stream())]
    res, spreads = {'shape': [B, T, H, DK]}, {}
    for name, (ms, spread) in zip(names, rounds_ms(fns, rounds, calls)):
        res[name + '_ms'], res[name + '_spread'], spreads[name] = round(ms, 4), [round(x, 4) for x in spread], spread
    for p in ('f32', 'bf16'):
        full = tiles_walked(host_lens, T, *hip.self_attn_tiles(p), None)
        for tag, win in windows.items():
            if win is None:
                continue
            walked = tiles_walked(host_lens, T, *hip.self_attn_tiles(p), win)
            # forward: key tiles; backward: the dQ kernel's key tiles and the dK/dV kernel's query tiles
            for d, frac in (('fwd', walked[0] / full[0]), ('bwd', (walked[0] + walked[1]) / (full[0] + full[1]))):
                key = '%s_%s_%s' % (d, tag, p)
                res[key + '_over_plain'] = round(res[key + '_ms'] / res['%s_plain_%s_ms' % (d, p)], 3)
                res[key + '_tiles_fraction'] = round(frac, 3)
                if tag != 'cT':
                    res[key + '_bar'] = 'met' if res[key + '_ms'] <= res['%s_plain_%s_ms' % (d, p)] else 'missed'
        if parent is not None:
            for d in ('fwd', 'bwd'):
                (a, (alo, ahi)), (b, (blo, bhi)) = ((res['%s_%s_%s_ms' % (d, s, p)], spreads['%s_%s_%s' % (d, s, p)]) for s in ('plain', 'parent'))
                res['%s_%s_plain_over_parent' % (d, p)] = round(a / b, 4)
                res['%s_%s_plain_bar' % (d, p)] = 'met' if alo <= b <= ahi or blo <= a <= bhi else 'missed'
    return res


def step_bench(rounds, calls):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    data = SyntheticData(8, 200, 123, min_frames=120, min_labels=5, max_labels=20, time_reduction=4, seed=2234)
    trainers = []
    for recipe in ('transformer_ctc', 'vgg_dblstm_ctc'):
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
    (tf, ts), (vgg, vs_) = rounds_ms([stepper(0), stepper(1)], rounds, calls)
    return {'shape': [8, 200, 123], 'transformer_ctc_step_ms': round(tf, 3), 'transformer_spread': [round(v, 3) for v in ts],
            'vgg_dblstm_step_ms': round(vgg, 3), 'vgg_spread': [round(v, 3) for v in vs_],
            'transformer_over_vgg_dblstm': round(tf / vgg, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--bf16', action='store_true', help='the bf16 kernels against the fp32 kernels and bf16 SDPA, nothing else')
    ap.add_argument('--dropout', action='store_true', help='the attention-dropout kernels against the plain kernels plus '
                    'separate dropout passes, nothing else')
    ap.add_argument('--window', action='store_true', help='the chunk-window kernels against the plain kernels on the same '
                    'operands, nothing else')
    ap.add_argument('--parent-lib', default=None, help='with --dropout or --window: a libnabu_hip.so built from the parent commit, whose '
                    'plain kernels are timed beside this build\'s')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'self_attn_bench needs a GPU'
    torch.cuda.set_device(0)
    if args.dropout or args.window:
        parent = None
        if args.parent_lib:
            import ctypes
            from nabu_amd import _hip
            parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
            for stem in ('nabu_self_attn', 'nabu_self_attn_bf16'):
                for what in ('_fwd', '_bwd'):
                    getattr(parent, stem + what).restype, getattr(parent, stem + what).argtypes = _hip.SIGNATURES[stem + what]
        bench = attn_window_bench if args.window else attn_dropout_bench
        res = {'bench': 'self_attn_window' if args.window else 'self_attn_dropout', 'rounds': args.rounds, 'calls': args.calls,
               'device': torch.cuda.get_device_name(0), 'parent_lib': bool(parent),
               'attention': [bench(T, args.rounds, args.calls, parent) for T in (250, 1000)]}
    elif args.bf16:
        res = {'bench': 'self_attn_bf16', 'rounds': args.rounds, 'calls': args.calls, 'device': torch.cuda.get_device_name(0),
               'attention': [attn_bf16_bench(T, args.rounds, args.calls) for T in (250, 1000)]}
    else:
        res = {'bench': 'self_attn', 'rounds': args.rounds, 'calls': args.calls, 'device': torch.cuda.get_device_name(0),
               'attention': [attn_bench(T, args.rounds, args.calls) for T in (250, 1000)],
               'step': step_bench(args.rounds, args.calls)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fid:
            fid.write(line + '\n')


if __name__ == '__main__':
    main()
