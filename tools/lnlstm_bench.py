"""Timing of one layer-normalised BLSTM layer (layer.blstm(layer_norm=True), nabu_blstm_ln_fwd / _bwd) at the four
layer shapes of cfg2 (B = 32, 512 units; T x D = 1000 x 40, 500 x 2048, 250 x 2048, 125 x 2048), forward + backward,
against the yardstick: the stepwise exact-fp32 layer WITHOUT layer norm at the same shape (LSTM_MODE = NABU_LSTM_STEPWISE,
recurrent_precision = f32) — the family the layer-normalised kernels belong to.

Protocol: both layers are warmed up at every shape, then timed alternately (one call of each per repetition) with device
events around forward + backward; the medians are reported.  Launches per step come from a run of its own under
`rocprofv3 --kernel-trace --stats` (a fresh child process; tracing slows the host, so nothing timed comes from it): the
calls of every ln_* kernel divided by the steps of the traced passes.

    python tools/lnlstm_bench.py [--reps 10] [--precision f16x3] [--no-trace] [--out DIR]

Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nabu_amd import ops as hip                                               # noqa: E402

B, H = 32, 512
SHAPES = [(1000, 40), (500, 2048), (250, 2048), (125, 2048)]
TRACE_PASSES = 2


class Layer(object):
    """buffers and the two calls (forward, backward) of one layer at one shape"""

    def __init__(self, T, D, layer_norm, precision, seed=0):
        rng = np.random.default_rng(seed)
        self.T, self.ln = T, layer_norm
        lens = rng.integers(T // 2, T + 1, B).astype(np.int32)
        lens[0] = T
        self.lens = torch.from_numpy(lens).cuda()
        lim = np.sqrt(6.0 / (D + 5 * H))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()      # noqa: E731
        self.x = dev(rng.standard_normal((B, T, D)))
        self.dout = dev(rng.standard_normal((B, T, 2 * H)))
        self.k = [dev(rng.uniform(-lim, lim, (D + H, 4 * H))) for _ in range(2)]
        self.dk = [torch.empty_like(k) for k in self.k]
        self.out = torch.empty((B, T, 2 * H), device='cuda')
        self.dx = torch.empty_like(self.x)
        if layer_norm:
            self.plan = hip.BlstmLnPlan(B, T, D, H, T, hip.LSTM_AUTO, precision)
            self.gam = [[torch.ones(H, device='cuda') for _ in range(5)] for _ in range(2)]
            self.bet = [[torch.zeros(H, device='cuda') for _ in range(5)] for _ in range(2)]
            self.dgam = [[torch.empty(H, device='cuda') for _ in range(5)] for _ in range(2)]
            self.dbet = [[torch.empty(H, device='cuda') for _ in range(5)] for _ in range(2)]
        else:
            self.plan = hip.BlstmPlan(B, T, D, H, T, hip.LSTM_STEPWISE, precision, recurrent_precision='f32')
            self.b = [torch.zeros(4 * H, device='cuda') for _ in range(2)]
            self.db = [torch.empty(4 * H, device='cuda') for _ in range(2)]
        self.reserve = torch.empty(self.plan.reserve_bytes, dtype=torch.uint8, device='cuda')

    def fwd_bwd(self):
        k, dk = self.k, self.dk
        if self.ln:
            hip.blstm_ln_fwd(self.plan, self.x, self.lens, k[0], k[1], self.gam, self.bet, self.out, self.reserve)
            hip.blstm_ln_bwd(self.plan, self.x, self.lens, k[0], k[1], self.gam, self.bet, self.out, self.dout, self.reserve,
                             self.dx, dk[0], dk[1], self.dgam, self.dbet)
        else:
            hip.blstm_fwd(self.plan, self.x, self.lens, k[0], self.b[0], k[1], self.b[1], self.out, self.reserve)
            hip.blstm_bwd(self.plan, self.x, self.lens, k[0], k[1], self.out, self.dout, self.reserve, self.dx, dk[0], self.db[0],
                          dk[1], self.db[1])


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def traced_child(args):
    """the child under rocprofv3: TRACE_PASSES forward + backward passes of the layer-normalised layer per shape"""
    for T, D in SHAPES:
        layer = Layer(T, D, True, args.precision)
        for _ in range(TRACE_PASSES):
            layer.fwd_bwd()
    torch.cuda.synchronize()


def launches_per_step(args):
    outdir = os.path.join(args.out, 'trace')
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', outdir, '-o', 'lnlstm', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--traced-child', '--precision', args.precision]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    if r.returncode != 0:
        raise RuntimeError('rocprofv3 run failed:\n' + r.stdout.decode(errors='replace')[-2000:])
    files = glob.glob(os.path.join(outdir, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise RuntimeError('rocprofv3 wrote no kernel_stats.csv under %s' % outdir)
    steps = TRACE_PASSES * sum(T for T, _ in SHAPES)
    calls = {'fwd': 0, 'bwd': 0}
    per_kernel = {}
    with open(files[0]) as fid:
        for row in csv.DictReader(fid):
            name = row['Name']
            for key in ('ln_rec_fwd_kernel', 'ln_cell_fwd_kernel', 'ln_rec_bwd_kernel', 'ln_cell_bwd_kernel',
                        'ln_param_grad_kernel'):
                if key in name:
                    per_kernel[key] = {'calls': int(row['Calls']), 'avg_us': round(float(row['AverageNs']) / 1e3, 2)}
                    if key != 'ln_param_grad_kernel':
                        calls['fwd' if 'fwd' in key else 'bwd'] += int(row['Calls'])
    return {'steps_traced': steps, 'fwd_launches_per_step': round(calls['fwd'] / steps, 4),
            'bwd_launches_per_step': round(calls['bwd'] / steps, 4), 'kernels': per_kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--precision', default='f16x3', help='gemm_precision of both layers (cfg2: f16x3)')
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--out', default=None, help='directory for the trace files (default: a temporary directory)')
    ap.add_argument('--traced-child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'lnlstm_bench needs a GPU'
    torch.cuda.set_device(0)
    if args.traced_child:
        return traced_child(args)
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix='lnlstm_bench_')
    rows = []
    for T, D in SHAPES:
        ln, plain = Layer(T, D, True, args.precision), Layer(T, D, False, args.precision)
        for _ in range(2):
            ln.fwd_bwd()
            plain.fwd_bwd()
        torch.cuda.synchronize()
        t_ln, t_plain = [], []
        for _ in range(args.reps):                      # alternating: both see the same neighbours and clocks
            t_plain.append(timed_once(plain.fwd_bwd))
            t_ln.append(timed_once(ln.fwd_bwd))
        m_ln, m_plain = float(np.median(t_ln)), float(np.median(t_plain))
        rows.append({'T': T, 'D': D, 'layer_norm_ms': round(m_ln, 3), 'stepwise_f32_ms': round(m_plain, 3),
                     'ratio': round(m_ln / m_plain, 3), 'layer_norm_min_max_ms': [round(min(t_ln), 3), round(max(t_ln), 3)],
                     'stepwise_min_max_ms': [round(min(t_plain), 3), round(max(t_plain), 3)]})
        del ln, plain
    res = {'bench': 'lnlstm_layer_fwd_bwd', 'B': B, 'H': H, 'precision': args.precision, 'reps': args.reps, 'layers': rows,
           'sum_layer_norm_ms': round(sum(r['layer_norm_ms'] for r in rows), 3),
           'sum_stepwise_f32_ms': round(sum(r['stepwise_f32_ms'] for r in rows), 3)}
    res['sum_ratio'] = round(res['sum_layer_norm_ms'] / res['sum_stepwise_f32_ms'], 3)
    if not args.no_trace:
        res['launches'] = launches_per_step(args)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
