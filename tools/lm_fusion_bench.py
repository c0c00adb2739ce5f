"""Timing of label n-gram fusion in both beam searches (lm_file / lm_weight):
(a) the CTC prefix beam search at [32, 125, 40], beam 100 — the decoder of cfg1 and cfg2 — without the LM and with a
    trigram (lm_weight 0.8, insertion_bonus 0.5);
(b) the 40-step attention beam search at the cfg3 decoder's geometry (B = 32, W = 16, Te = 125, C = 40) without the
    LM and with the trigram (lm_weight 0.5);
(c) the same two searches WITHOUT the LM on the parent commit (--parent-root DIR, a checkout of it with its library
    built) — the condition is on these: each plain leg of this tree must agree with the parent's within the spread the
    parent's own repetitions show.  The fused legs are reported, not gated;
(d) the pruning step on its own with and without the LM term, and the kernel launches of one attention search with and
    without the LM (torch.profiler): the LM adds none per step.

Protocol (tools/joint_ctc_bench.py): every measurement runs in a child process of its own tree, everything is warmed
up, the arms of a child are timed alternately, one call of each per repetition; the children alternate over --rounds
rounds (their order reversed every other round); medians are reported with the spread of the rounds.  The plain legs are
compared like for like: the same two-arm child on the parent's tree and on this one; the fused legs run in a four-arm
child of this tree, next to its own plain arms.

    python tools/lm_fusion_bench.py [--reps 20] [--rounds 5] [--parent-root DIR] [--out profiles/lm_fusion.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTC = dict(B=32, T=125, C=40, W=100, order=3, lm_weight=0.8, insertion_bonus=0.5)
ATT = dict(B=32, W=16, Te=125, C=40, S=40, order=3, lm_weight=0.5)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def trigram(C, order, dev):
    """a model estimated from seeded random sentences over the C - 1 labels"""
    from nabu_amd.processing import ngram_lm
    rng = np.random.default_rng(11)
    sentences = [rng.integers(0, C - 1, rng.integers(5, 40)).tolist() for _ in range(2000)]
    return ngram_lm.train(sentences, ['s%d' % i for i in range(C - 1)], order)


def legs_child(with_lm, reps):
    """in a child process, on the tree at the head of sys.path: the plain legs, and with `with_lm` the fused ones, timed
    alternately.  Only calls that exist on the parent commit are made without `with_lm`."""
    from nabu_amd import ops, recipes, variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory, rnn_decoder
    dev = torch.device('cuda')
    gen = torch.Generator(device='cuda').manual_seed(7)
    c = CTC
    logits = 2.0 * torch.randn((c['B'], c['T'], c['C']), device=dev, generator=gen)
    lens = torch.full((c['B'],), c['T'], dtype=torch.int32, device=dev)
    a = ATT
    mc, _, _ = recipes.load_recipe('cfg3_las_vanilla')
    dec = ed_decoder_factory.factory('speller')(mc, {'text': a['C']}, None)
    E = 2 * int(mc.get('encoder', 'num_units'))
    enc = torch.randn((a['B'], a['Te'], E), device=dev, generator=gen)
    enc_len = np.full(a['B'], a['Te'], np.int32)
    store = vs.VariableStore(seed=5)
    arms = {'ctc_plain': lambda: ops.ctc_beam_search(logits, lens, c['W'], True)}
    with torch.no_grad(), vs.as_default(store), vs.variable_scope(dec.scope):
        cell = dec.create_cell({'features': enc}, {'features': SeqLen(enc_len, dev)}, False)
        rnn_decoder.cell_parameters(cell, E)
        store.vars['Speller/decoder/dense/bias'].data[a['C'] - 1] = -30.0     # no hypothesis ends: all S steps run
        args = (cell, enc, SeqLen(enc_len, dev), a['W'], a['S'], 1.0, 1.0, False)
        steps = {}

        def attention(name, **kw):
            def run():
                steps[name] = int(rnn_decoder.beam_search(*args, **kw)[0].shape[2])
            return run
        arms['attention_plain'] = attention('attention_plain')
        if with_lm:
            lm = trigram(c['C'], c['order'], dev)
            table = lm.device_table(dev)
            arms['ctc_lm'] = lambda: ops.ctc_beam_search_lm(logits, lens, table, lm.order, c['lm_weight'],
                                                            c['insertion_bonus'], c['W'], True)
            arms['attention_lm'] = attention('attention_lm', lm=lm, lm_weight=a['lm_weight'])
        for _ in range(3):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                t[k].append(wall_ms(fn))
        out = {'ms': {k: round(float(np.median(v)), 4) for k, v in t.items()}, 'steps': steps}
        if with_lm:
            out.update(prune_and_launches(arms, logits.device, gen, lm, reps))
    print('LEGS ' + json.dumps(out), flush=True)


def prune_and_launches(arms, dev, gen, lm, reps):
    """(d): the pruning step with and without the LM term, and the kernels of one attention search of each kind"""
    from nabu_amd import ops
    a = ATT
    B, W, C = a['B'], a['W'], a['C']
    logits = torch.randn((B, W, C), device=dev, generator=gen)
    zeros = torch.zeros((B, W), dtype=torch.int32, device=dev)
    ctx = torch.randint(0, lm.num_contexts, (B, W), device=dev, generator=gen).to(torch.int32)
    table = lm.device_table(dev)

    def prune(fused):
        st = [-torch.rand((B, W), device=dev), zeros.clone(), zeros.clone(), zeros.clone()]
        if fused:
            return lambda: ops.beam_prune_lm(logits, None, 0.0, table, lm.order, a['lm_weight'], ctx, *st, 1.0, 1.0)
        return lambda: ops.beam_prune(logits, *st, 1.0, 1.0)
    calls = {'beam_prune': prune(False), 'beam_prune_lm': prune(True)}
    for _ in range(5):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(max(reps, 20)):
        for k, fn in calls.items():
            t[k].append(timed_once(fn))
    out = {'prune_us': {k: round(1e3 * float(np.median(v)), 2) for k, v in t.items()}}
    try:
        from torch.profiler import ProfilerActivity, profile
        counts = {}
        for k in ('attention_plain', 'attention_lm'):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                arms[k]()
                torch.cuda.synchronize()
            counts[k] = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA')
                            and not e.name.lower().startswith(('memcpy', 'memset')))
        out['kernel_launches'] = counts
    except Exception as e:                                  # (a profiler that cannot attach: said, not hidden)
        out['kernel_launches'] = 'not counted: %s' % e
    return out


def run_child(root, with_lm, reps):
    cmd = [sys.executable, os.path.abspath(__file__), '--legs-child', '--root', root, '--reps', str(reps)]
    res = subprocess.run(cmd + (['--with-lm'] if with_lm else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=900)
    lines = [l for l in res.stdout.splitlines() if l.startswith('LEGS ')]
    if res.returncode != 0 or not lines:
        raise RuntimeError('measurement failed (%d): %s' % (res.returncode, res.stdout[-2000:]))
    return json.loads(lines[-1][5:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit, its library built')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_fusion.json'))
    ap.add_argument('--legs-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--with-lm', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lm_fusion_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, os.path.abspath(args.root))
    if args.legs_child:
        return legs_child(args.with_lm, args.reps)
    parent = args.parent_root and os.path.abspath(args.parent_root)
    # the plain legs like for like: the same two-arm child on both trees; the fused legs in a four-arm child of their own.
    # The order of the children is reversed every other round, so that no tree always runs behind the same neighbour.
    trees = ([('parent_commit', parent, False)] if parent else []) + [('this_tree', ROOT, False), ('this_tree_lm', ROOT, True)]
    ms = {name: {} for name, _, _ in trees}
    extra = {}
    for r in range(args.rounds):
        for name, root, with_lm in (trees if r % 2 == 0 else trees[::-1]):
            got = run_child(root, with_lm, args.reps)
            for k, v in got['ms'].items():
                ms[name].setdefault(k, []).append(v)
            if with_lm:
                extra = {k: got[k] for k in ('steps', 'prune_us', 'kernel_launches')}
        print('round %d: %s' % (r, {n: {k: v[-1] for k, v in m.items()} for n, m in ms.items()}), file=sys.stderr, flush=True)
    med = {n: {k: float(np.median(v)) for k, v in m.items()} for n, m in ms.items()}
    spread = {n: {k: round((max(v) - min(v)) / med[n][k], 4) for k, v in m.items()} for n, m in ms.items()}
    res = {'bench': 'lm_fusion', 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'ctc': CTC, 'attention': ATT, 'ms_per_round': ms,
           'median_ms': {n: {k: round(v, 4) for k, v in m.items()} for n, m in med.items()}, 'spread': spread}
    t, plain = med['this_tree_lm'], med['this_tree']
    S = max(extra['steps'].get('attention_lm', ATT['S']), 1)
    res['fused'] = {'ctc_lm_over_plain': round(t['ctc_lm'] / t['ctc_plain'], 4),
                    'ctc_added_us_per_frame': round(1e3 * (t['ctc_lm'] - t['ctc_plain']) / CTC['T'], 2),
                    'attention_lm_over_plain': round(t['attention_lm'] / t['attention_plain'], 4),
                    'attention_added_us_per_step': round(1e3 * (t['attention_lm'] - t['attention_plain']) / S, 2),
                    'steps_run': extra['steps'], 'prune_us': extra['prune_us'], 'kernel_launches': extra['kernel_launches']}
    if isinstance(extra['kernel_launches'], dict):
        k = extra['kernel_launches']
        res['fused']['launches_added_per_step'] = round((k['attention_lm'] - k['attention_plain'] - 1) / S, 4)   # (- the one fill)
    if parent:
        res['plain_legs'] = {}
        for k in ('ctc_plain', 'attention_plain'):
            p = ms['parent_commit'][k]
            res['plain_legs'][k] = {'this_over_parent': round(plain[k] / med['parent_commit'][k], 4),
                                    'parent_spread_ms': round(max(p) - min(p), 4),
                                    'difference_ms': round(plain[k] - med['parent_commit'][k], 4),
                                    'within_parent_spread': bool(abs(plain[k] - med['parent_commit'][k]) <= max(p) - min(p))}
    else:
        res['plain_legs'] = 'parent commit not measured (no --parent-root)'
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
