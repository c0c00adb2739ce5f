"""Timing of joint CTC/attention training and decoding (ctc_head / ctc_weight):
(a) the cfg3 training step with ctc_head = True and ctc_weight = 0.3 against the step without the keys, and the step
    without the keys against the parent commit's — the condition is that the last two agree within the spread the
    parent's own repetitions show;
(b) one beam search at the cfg3 decoder's geometry (B = 32, W = 16, Te = 125, C = 40, 40 steps) with ctc_weight = 0.3
    against the same search with ctc_weight = 0 (the plain launches);
(c) the launches the joint search adds, each on its own at that geometry: nabu_ctc_prefix_prepare (once per search),
    nabu_ctc_prefix_score and nabu_ctc_prefix_advance (per step), and nabu_beam_prune_joint next to nabu_beam_prune.

Protocol (tools/grad_norm_bench.py): everything is warmed up, candidates are timed alternately, one call of each per
repetition; medians are reported with the spread of the repetitions.  The training steps run in child processes, one per
measurement, alternating over --rounds rounds.  With --parent-root DIR (a checkout of the parent commit with its library
built) the baseline step is that checkout's; otherwise that leg is left out and the result says so.

    python tools/joint_ctc_bench.py [--reps 30] [--steps 20] [--rounds 3] [--parent-root DIR] [--no-step]
                                    [--out profiles/joint_ctc.json]

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
LAM = 0.3
GEO = dict(B=32, W=16, Te=125, C=40, S=40)
JOINT = {'decoder.ctc_head': 'True', 'trainer.ctc_weight': LAM}


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(t, unit=1.0, digits=4):
    return {'median': round(unit * float(np.median(t)), digits), 'min_max': [round(unit * min(t), digits),
                                                                            round(unit * max(t), digits)]}


# ------------------------------------------------------------------------------------------------ (a) training step
def step_child(joint, steps, warmup=3):
    """in a child process: `steps` training steps of cfg3 (bench.py's cfg3 batch) on one resident batch"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    mc, tc, ec = recipes.load_recipe('cfg3_las_vanilla', **(JOINT if joint else {}))
    data = SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=79, eos=True, time_reduction=8, seed=3234)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=None, task_index=0)
    batch = tr.to_device(data.batch(0))
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    t = [timed_once(lambda: tr.step(batch)) for _ in range(steps)]
    print('STEP ' + json.dumps({'joint': joint, 'steps': steps, 'step_ms': round(float(np.median(t)), 4),
                                'min_max_ms': [round(min(t), 4), round(max(t), 4)]}), flush=True)


def run_child(root, joint, steps):
    cmd = [sys.executable, os.path.abspath(__file__), '--step-child', '--root', root, '--steps', str(steps)]
    res = subprocess.run(cmd + (['--joint'] if joint else []), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    lines = [l for l in res.stdout.splitlines() if l.startswith('STEP ')]
    if res.returncode != 0 or not lines:
        raise RuntimeError('step measurement failed (%d): %s' % (res.returncode, res.stdout[-2000:]))
    return json.loads(lines[-1][5:])


def step_timing(parent_root, steps, rounds):
    arms = {'this_tree_without_keys': (ROOT, False), 'this_tree_joint': (ROOT, True)}
    if parent_root:
        arms = dict({'parent_commit': (parent_root, False)}, **arms)
    ms = {k: [] for k in arms}
    for r in range(rounds):
        for k, (root, joint) in arms.items():
            ms[k].append(run_child(root, joint, steps)['step_ms'])
        print('round %d: %s' % (r, {k: v[-1] for k, v in ms.items()}), file=sys.stderr, flush=True)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {'workload': 'cfg3, batch 32 x 1000 x 40', 'ctc_weight': LAM, 'steps_per_run': steps, 'rounds': rounds,
           'step_ms': ms, 'median_ms': {k: round(v, 4) for k, v in med.items()},
           'spread': {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
           'joint_over_without_keys': round(med['this_tree_joint'] / med['this_tree_without_keys'], 4)}
    if parent_root:
        out['without_keys_over_parent'] = round(med['this_tree_without_keys'] / med['parent_commit'], 4)
        out['without_keys_within_parent_spread'] = bool(
            abs(med['this_tree_without_keys'] - med['parent_commit']) <= max(ms['parent_commit']) - min(ms['parent_commit']))
    else:
        out['parent_commit'] = 'not measured (no --parent-root)'
    return out


# -------------------------------------------------------------------------------------- (b), (c) search and launches
def search_and_launches(reps):
    from nabu_amd import ops, recipes, variables as vs
    from nabu_amd.autodiff import SeqLen
    from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory, rnn_decoder
    g = GEO
    B, W, Te, C, S = g['B'], g['W'], g['Te'], g['C'], g['S']
    dev = torch.device('cuda')
    mc, _, _ = recipes.load_recipe('cfg3_las_vanilla')
    dec = ed_decoder_factory.factory('speller')(mc, {'text': C}, None)
    E = 2 * int(mc.get('encoder', 'num_units'))
    gen = torch.Generator(device='cuda').manual_seed(7)
    enc = torch.randn((B, Te, E), device=dev, generator=gen)
    enc_len = np.full(B, Te, np.int32)
    ctc_logits = 2.0 * torch.randn((B, Te, C), device=dev, generator=gen)
    store = vs.VariableStore(seed=5)
    out = {'geometry': dict(g, E=E, U=int(mc.get('decoder', 'num_units')))}
    with torch.no_grad(), vs.as_default(store), vs.variable_scope(dec.scope):
        cell = dec.create_cell({'features': enc}, {'features': SeqLen(enc_len, dev)}, False)
        rnn_decoder.cell_parameters(cell, E)
        store.vars['Speller/decoder/dense/bias'].data[C - 1] = -30.0     # no hypothesis ends: all S steps run
        args = (cell, enc, SeqLen(enc_len, dev), W, S, 1.0, 1.0, False)

        def search(lam):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seqs = rnn_decoder.beam_search(*args, ctc_logits=ctc_logits, ctc_weight=lam)[0]
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), int(seqs.shape[2])
        for lam in (0.0, LAM, 0.0, LAM):
            search(lam)
        times, steps = {0.0: [], LAM: []}, {}
        for _ in range(reps):
            for lam in (0.0, LAM):
                ms, n = search(lam)
                times[lam].append(ms)
                steps[lam] = n
    plain, joint = float(np.median(times[0.0])), float(np.median(times[LAM]))
    out['search'] = {'steps_run': {'plain': steps[0.0], 'joint': steps[LAM]}, 'plain_ms': stats(times[0.0]),
                     'joint_ms': stats(times[LAM]), 'joint_over_plain': round(joint / plain, 4),
                     'added_us_per_step': round(1e3 * (joint - plain) / max(steps[LAM], 1), 2),
                     'plain_spread': round((max(times[0.0]) - min(times[0.0])) / plain, 4)}
    # (c) the launches on their own: a beam of 10-label hypotheses (ten advance steps from the empty one)
    lens = torch.full((B,), Te, dtype=torch.int32, device=dev)
    s = ops.ctc_prefix_prepare(ctc_logits, lens, W)
    zeros = torch.zeros((B, W), dtype=torch.int32, device=dev)
    parent = torch.arange(W, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    for k in range(10):
        pred = ((parent * 7 + 3 * k) % (C - 1)).to(torch.int32).contiguous()
        s = ops.ctc_prefix_advance(s, parent, zeros, pred)
    delta = ops.ctc_prefix_score(s, zeros)
    logits = torch.randn((B, W, C), device=dev, generator=gen)

    def prune(joint_):
        lp = -torch.rand((B, W), device=dev)
        st = [lp, zeros.clone(), zeros.clone(), zeros.clone()]
        if joint_:
            return lambda: ops.beam_prune_joint(logits, delta, LAM, *st, 1.0, 1.0)
        return lambda: ops.beam_prune(logits, *st, 1.0, 1.0)
    calls = {'ctc_prefix_prepare': lambda: ops.ctc_prefix_prepare(ctc_logits, lens, W),
             'ctc_prefix_score': lambda: ops.ctc_prefix_score(s, zeros),
             'ctc_prefix_advance': lambda: ops.ctc_prefix_advance(s, parent, zeros, pred),
             'beam_prune_joint': prune(True), 'beam_prune': prune(False)}
    for _ in range(5):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t[k].append(timed_once(fn))
    out['launches_us'] = {k: stats(v, 1e3, 2) for k, v in t.items()}
    per_step = sum(out['launches_us'][k]['median'] for k in ('ctc_prefix_score', 'ctc_prefix_advance', 'beam_prune_joint'))
    out['launches_us']['per_step_added'] = round(per_step - out['launches_us']['beam_prune']['median'], 2)
    out['launches_us']['note'] = ('each call timed between two device events, with the allocation of its outputs; the '
                                  'search makes the same launches from a workspace')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit, its library built')
    ap.add_argument('--no-step', action='store_true', help='the search and launch timings only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'joint_ctc.json'))
    ap.add_argument('--step-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--joint', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'joint_ctc_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, os.path.abspath(args.root))
    if args.step_child:
        return step_child(args.joint, args.steps)
    res = {'bench': 'joint_ctc', 'reps': args.reps, 'device': torch.cuda.get_device_name(0)}
    res.update(search_and_launches(args.reps))
    if not args.no_step:
        res['cfg3_step'] = step_timing(args.parent_root and os.path.abspath(args.parent_root), args.steps, args.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
