"""Timing of minimum word error rate training on the device (mwer_nbest): (a) nabu_mwer_loss_grad at the cfg3 decoder's
geometry (B 32, N 4, L 45, C 40) next to nabu_xent_loss_grad on the same stacked logits, which is its bar (at most 2 x:
it reads the logits twice and writes the same gradient); (b) the tile, tile-backward and prepare launches, each on its
own; (c) the cfg3 training step with mwer_nbest = 4 against the plain cfg3 step, and the plain step against the parent
commit's.

Protocol (tools/grad_norm_bench.py): everything is warmed up; a round is --reps calls of one candidate between two device
events, the candidates of a group alternate round by round, and the median of --rounds rounds is reported with their
spread.  The steps run in child processes, one per measurement, alternating parent / plain / MWER for --rounds rounds.
With --parent-root DIR (a checkout of the parent commit with its library built) the parent's step is that checkout's;
otherwise that comparison is left out and the result says so.

    python tools/mwer_bench.py [--reps 200] [--rounds 5] [--steps 15] [--parent-root DIR] [--no-step]
                               [--out profiles/mwer.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = dict(B=32, N=4, L=45, C=40)
ENCODED = dict(B=32, Te=125, E=1024)            # the cfg3 listener's output for 1000 frames: 125 x (2 x 512)
NBEST, MAX_STEPS = 4, 80                        # the step: the references of bench.py's cfg3 leg have up to 80 labels


def timed_round(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps       # us per call


def measure(groups, reps, rounds):
    """groups: lists of (name, fn); the members of a group alternate round by round -> {name: [us per round]}"""
    times = {}
    for group in groups:
        for _, fn in group:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in group:
                times.setdefault(name, []).append(timed_round(fn, reps))
    return times


def launches(reps, rounds):
    from nabu_amd import ops as hip
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(7)
    B, N, L, C = (GEOMETRY[k] for k in 'BNLC')
    rows = (N + 1) * B
    logits = (torch.randn((rows, L, C), generator=g) * 2.0).to(dev)
    targets = torch.randint(0, C, (rows, L), generator=g, dtype=torch.int32).to(dev)
    lens = torch.randint(20, L + 1, (rows,), generator=g, dtype=torch.int32).to(dev)
    errors = torch.randint(0, 30, (N * B,), generator=g, dtype=torch.int32).to(dev)
    valid = torch.ones(N * B, dtype=torch.int32, device=dev)
    enc = torch.randn((ENCODED['B'], ENCODED['Te'], ENCODED['E']), generator=g).to(dev)
    denc = torch.randn(((N + 1) * ENCODED['B'], ENCODED['Te'], ENCODED['E']), generator=g).to(dev)
    seq = torch.randint(0, C - 1, (B, N, L), generator=g, dtype=torch.int32).to(dev)
    seq_len = torch.randint(20, L, (B, N), generator=g, dtype=torch.int32).to(dev)
    scores = -torch.rand((B, N), generator=g).to(dev)
    ref = torch.randint(0, C - 1, (B, L), generator=g, dtype=torch.int32).to(dev)
    ref_len = torch.randint(20, L + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    groups = [[('mwer_loss_grad', lambda: hip.mwer_loss_grad(logits, targets, lens, errors, valid, 0.01, 1.0 / B)),
               ('xent_loss_grad', lambda: hip.xent_loss_grad(logits, targets, lens, lens, 1.0 / rows))],
              [('rows_tile', lambda: hip.rows_tile(enc, N + 1))],
              [('rows_tile_bwd', lambda: hip.rows_tile_bwd(denc, N + 1))],
              [('mwer_prepare', lambda: hip.mwer_prepare(seq, seq_len, scores, ref, ref_len, C))]]
    times = measure(groups, reps, rounds)
    row = dict(GEOMETRY, encoded=ENCODED, reps_per_round=reps, rounds=rounds,
               note='a call is the Python wrapper: the launch and the allocation of its outputs')
    for name, t in times.items():
        row[name + '_us'] = round(float(np.median(t)), 2)
        row[name + '_min_max_us'] = [round(min(t), 2), round(max(t), 2)]
    row['mwer_over_xent'] = round(row['mwer_loss_grad_us'] / row['xent_loss_grad_us'], 3)
    row['within_the_2x_bar'] = bool(row['mwer_over_xent'] <= 2.0)
    moved = 4.0 * enc.numel() * (N + 2)          # one copy read, N + 1 written (backward: the reverse)
    row['rows_tile_gb_per_s'] = round(moved / row['rows_tile_us'] / 1e3, 1)
    row['rows_tile_bwd_gb_per_s'] = round(moved / row['rows_tile_bwd_us'] / 1e3, 1)
    return row


def trainer(mwer):
    """a cfg3 trainer on the batch source of bench.py's cfg3 leg (the package comes from sys.path[0])"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    over = {'trainer.mwer_nbest': NBEST, 'trainer.mwer_max_steps': MAX_STEPS} if mwer else {}
    mc, tc, ec = recipes.load_recipe('cfg3_las_vanilla', **over)
    data = SyntheticData(32, 1000, 40, min_frames=1000, min_labels=20, max_labels=79, eos=True, time_reduction=8, seed=3234)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0), data


def step_child(mwer, steps, warmup=3):
    """in a child process: `steps` training steps of cfg3 on one resident batch, each between two device events"""
    from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
    tr, data = trainer(mwer)
    batch = tr.to_device(data.batch(0))
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.step(batch)
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    out = {'mwer': bool(mwer), 'steps': steps, 'step_ms': round(float(np.median(t)), 4),
           'min_max_ms': [round(min(t), 4), round(max(t), 4)]}
    desc = rnn_decoder.dynamic_decode.last[0]
    out['decoder_rows'], out['decoder_steps'] = int(desc.B), int(desc.L)
    out['decoder_paths_fwd_bwd'] = [int(p) for p in rnn_decoder.dynamic_decode.last_paths]
    if mwer:
        out['mwer_stats'] = list(tr.mwer_stats())
    print('STEP ' + json.dumps(out), flush=True)


def run_child(root, mwer, steps):
    cmd = [sys.executable, os.path.abspath(__file__), '--step-child', '--root', root, '--steps', str(steps)]
    if mwer:
        cmd.append('--mwer')
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in res.stdout.splitlines() if l.startswith('STEP ')]
    if res.returncode != 0 or not lines:
        raise RuntimeError('step measurement failed (%d): %s' % (res.returncode, res.stdout[-2000:]))
    return json.loads(lines[-1][5:])


def step_timing(parent_root, steps, rounds):
    runs = {'parent': [], 'plain': [], 'mwer': []}
    for r in range(rounds):
        if parent_root:
            runs['parent'].append(run_child(parent_root, False, steps))
        runs['plain'].append(run_child(ROOT, False, steps))
        runs['mwer'].append(run_child(ROOT, True, steps))
        print('round %d: %s' % (r, {k: v[-1]['step_ms'] for k, v in runs.items() if v}), file=sys.stderr, flush=True)
    out = {'workload': 'cfg3, batch 32 x 1000 x 40', 'mwer_nbest': NBEST, 'mwer_max_steps': MAX_STEPS,
           'steps_per_run': steps, 'rounds': rounds}
    for k, v in runs.items():
        if not v:
            continue
        ms = [x['step_ms'] for x in v]
        out[k + '_ms'] = ms
        out[k + '_median_ms'] = round(float(np.median(ms)), 4)
        out[k + '_spread'] = round((max(ms) - min(ms)) / float(np.median(ms)), 4)
    out['mwer_over_plain'] = round(out['mwer_median_ms'] / out['plain_median_ms'], 3)
    last = runs['mwer'][-1]
    out['mwer_decoder_pass'] = {k: last[k] for k in ('decoder_rows', 'decoder_steps', 'decoder_paths_fwd_bwd')}
    out['plain_decoder_pass'] = {k: runs['plain'][-1][k] for k in ('decoder_rows', 'decoder_steps', 'decoder_paths_fwd_bwd')}
    out['decoder_paths_legend'] = '1: the persistent decoder kernel, 0: one launch chain per step'
    out['mwer_stats_last_step'] = last.get('mwer_stats')
    if runs['parent']:
        p = [x['step_ms'] for x in runs['parent']]
        out['plain_over_parent'] = round(out['plain_median_ms'] / out['parent_median_ms'], 4)
        out['plain_inside_the_parents_spread'] = bool(min(p) <= out['plain_median_ms'] <= max(p))
    else:
        out['parent'] = 'not measured (no parent checkout given)'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--parent-root', default=None, help='a checkout of the parent commit, its library built')
    ap.add_argument('--no-step', action='store_true', help='the launch timings only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mwer.json'))
    ap.add_argument('--step-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument('--mwer', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'mwer_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, os.path.abspath(args.root))
    if args.step_child:
        return step_child(args.mwer, args.steps)
    res = {'bench': 'mwer', 'device': torch.cuda.get_device_name(0), 'launches': launches(args.reps, args.rounds)}
    if not args.no_step:
        res['cfg3_step'] = step_timing(args.parent_root and os.path.abspath(args.parent_root), args.steps, args.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
