"""Timing of the transducer kernels (csrc/transducer.hip) against the CTC loss launch (nabu_ctc_loss_grad) IN THE SAME RUN
on the same B, T, C and labels, at the shapes tools/ctc_align_bench.py uses:
    [32, 125, 40] with L ~ 40
    [32, 1000, 40] with L ~ 50
Per shape: the sweep launch on its own (NABU_TRANSDUCER_LAUNCHES=2 on a workspace a complete call has filled), the whole
call, the CTC call, and one greedy decoding step (nabu_transducer_greedy_step).
The bar is on the sweep launch: no longer than (T + U1) / T times the CTC launch at the same shape — per chain step it
does the work of the CTC wave kernel (a two-term log-sum-exp and an emission on one wave) on a chain longer by that
factor, and the CTC launch also does its softmax and its gradient.  The whole call's ratio to CTC is reported without a
bar.  With --steps the training step of the transducer recipe at cfg1's size (8 x 200 x 40, 10 .. 40 labels) is timed
against the cfg1 CTC step, alternated in the same way.

Protocol: everything is warmed up; a round times the arms alternately, one call of each per repetition, between device
events, and keeps the median of each; medians of --rounds rounds are reported with the spread of the rounds
((max - min) / median).

    python tools/transducer_bench.py [--reps 200] [--rounds 5] [--steps 20] [--out profiles/transducer.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [dict(B=32, T=125, C=40, L=40), dict(B=32, T=1000, C=40, L=50)]
SWITCH = 'NABU_TRANSDUCER_LAUNCHES'


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds_of(arms, reps, rounds, scale=1e3):
    """medians per round of every arm (alternated), in microseconds (scale 1e3) -> (per_round, median, spread)"""
    per_round = {k: [] for k in arms}
    for _ in range(rounds):
        t = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                t[k].append(timed_once(fn))
        for k in arms:
            per_round[k].append(scale * float(np.median(t[k])))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    return ({k: [round(x, 2) for x in v] for k, v in per_round.items()}, {k: round(v, 2) for k, v in med.items()},
            {k: round((max(v) - min(v)) / med[k], 4) for k, v in per_round.items()})


def operands(shape, dev):
    """ctc_align_bench's operands (seeded N(0, 2) logits, full-length utterances, label lengths within 10 % of L) plus
    prediction logits g [B, Lmax + 1, C] drawn the same way"""
    B, T, C, L = shape['B'], shape['T'], shape['C'], shape['L']
    rng = np.random.default_rng(1000 * T + L)
    Lmax = L + L // 10
    label_len = rng.integers(L - L // 10, Lmax + 1, B).astype(np.int32)
    labels = rng.integers(0, C - 1, (B, Lmax)).astype(np.int32)
    logits = (2.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    g = (2.0 * rng.standard_normal((B, Lmax + 1, C))).astype(np.float32)
    return (torch.tensor(logits, device=dev), torch.tensor(g, device=dev),
            torch.full((B,), T, dtype=torch.int32, device=dev), torch.tensor(labels, device=dev),
            torch.tensor(label_len, device=dev))


def measure(shape, reps, rounds):
    from nabu_amd import ops
    dev = torch.device('cuda')
    f, g, enc_len, labels, label_len = operands(shape, dev)
    B, T, C = f.shape
    U1, S = g.shape[1], 64

    def whole():
        return ops.transducer_loss_grad(f, g, enc_len, labels, label_len, 1.0 / B)

    def sweep():
        os.environ[SWITCH] = '2'
        try:
            return whole()
        finally:
            os.environ[SWITCH] = '7'
    state = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
    ids, score, g_row = torch.zeros((B, S), dtype=torch.int32, device=dev), torch.zeros(B, device=dev), g[:, 0].contiguous()
    arms = {'sweep': sweep, 'transducer': whole,
            'ctc': lambda: ops.ctc_loss_grad(f, enc_len, labels, label_len, 1.0 / B),
            # step 0 sets the search state up and decides at frame 0: the state never runs out of frames
            'greedy_step': lambda: ops.transducer_greedy_step(0, f, g_row, enc_len, state[0], state[1], ids, state[2],
                                                              state[3], score)}
    ref = whole()
    assert int(ref[3].item()) == 0 and int(arms['ctc']()[2].item()) == 0
    again = sweep()                       # the sweeps alone, on the workspace the complete call filled: the same nll
    assert torch.equal(again[0], ref[0])
    for _ in range(10):
        for fn in arms.values():
            fn()
    per_round, med, spread = rounds_of(arms, reps, rounds)
    bar = (T + U1) / float(T)
    return {'shape': dict(shape, U1=U1), 'us_per_round': per_round, 'median_us': med, 'spread': spread,
            'sweep_over_ctc': round(med['sweep'] / med['ctc'], 4), 'bar': round(bar, 4),
            'bar_met': bool(med['sweep'] <= bar * med['ctc']),
            'transducer_over_ctc': round(med['transducer'] / med['ctc'], 4)}


def measure_steps(reps, rounds):
    """the training step of dblstm_transducer_timit against cfg1_dblstm_ctc's, both at cfg1's size, in milliseconds"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    arms = {}
    for name, recipe in (('transducer', 'dblstm_transducer_timit'), ('ctc', 'cfg1_dblstm_ctc')):
        data = SyntheticData(8, 200, 40, min_frames=200, min_labels=10, max_labels=40, seed=1234)
        mc, tc, ec = recipes.load_recipe(recipe)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                 server=None, task_index=0)
        batch = tr.to_device(data.batch(0))
        arms[name] = lambda tr=tr, batch=batch: tr.step(batch)
    for _ in range(3):
        for fn in arms.values():
            fn()
    per_round, med, spread = rounds_of(arms, reps, rounds, scale=1.0)
    return {'workload': '8 x 200 x 40 fbank, 10 .. 40 labels, DBLSTM 2 x 256', 'ms_per_round': per_round, 'median_ms': med,
            'spread': spread, 'transducer_over_ctc': round(med['transducer'] / med['ctc'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20, help='training steps per round of the recipe comparison; 0 skips it')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transducer.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'transducer_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, ROOT)
    res = {'bench': 'transducer', 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'route': 'workgroup' if os.environ.get('NABU_TRANSDUCER_WORKGROUP', '0') not in ('', '0') else 'default',
           'cases': [measure(s, args.reps, args.rounds) for s in SHAPES]}
    if args.steps:
        res['training_step'] = measure_steps(args.steps, args.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
