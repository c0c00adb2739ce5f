#!/usr/bin/env python
"""bench.py — utterances/sec of the Nabu training step on MI355X.

  python bench.py --gpus N --steps K --warmup W [--full]
  N > 1 either way:
    * python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
      --master-port P bench.py --gpus N ...      (ranks are given: RANK/WORLD_SIZE in the env)
    * python bench.py --gpus N ...               (no WORLD_SIZE in the env: bench.py starts its own
      N ranks on this node through torch.distributed.run over 127.0.0.1 — the analogue of the
      reference's single_machine local cluster, nabu/scripts/prepare_train.py:107-123,
      nabu/computing/local_cluster.py:22-41)

Workload (BASELINE.json configs[1]/[3], "cfg2"): 4-layer Listener-512 (3 pyramidal
BLSTM layers + 1 BLSTM) + DNNDecoder + CTC, batch 32 x 1000 frames x 40 fbank per
GPU, fp32, synthetic seeded data, random-init weights.  One step = forward + CTC
loss/gradient + backward + per-element clip + Adam (+ RCCL all-reduce of the
clipped gradients when N > 1, weak scaling: every rank has its own batch of 32).
Inputs are resident in HBM before the timed region.

Arithmetic of the dense products (--gemm-precision): the headline runs them as fp32-EQUIVALENT
products on the 16-bit matrix pipe — f16x3: every operand row scaled by a power of two and held as
two fp16 planes, three plane products, 16-k partial sums promoted to fp32 accumulators; measured
error against float64 at or below the exact-fp32 MFMA kernel's (tests/test_hip_gemm_pk.py), per-step
loss within 5e-5 of the float64 oracle at the full size (tests/test_hip_golden.py) — everything else
of the step is fp32.  A --full run times the same step with the exact six-plane split on the bf16 pipe (bf16x6)
and with exact-fp32 products (v_mfma_f32_32x32x2_f32) after the headline and prints them as the `alt_bf16x6`
and `f32_products` objects of the line, and once more as `fp32_end_to_end`: exact-fp32 products AND the exact-fp32
recurrent kernels (the headline's recurrent product runs as three fp16 plane products of row-scaled operands).

One JSON line is printed by rank 0.  A plain run sets up, warms up, times the K steps, writes its outputs if
--dump-outputs is given and prints the line; what it reports beyond the headline comes from those steps:
  roofline     — SURVEY.md 8(d): the recurrent LSTM step's ALGORITHMIC bytes (per timestep per
                 direction W_h + x-projection + gate activations + h/c state) of a whole
                 training step over the measured step time = `frac` of the HBM peak; the
                 recurrent kernels alone (HIP events recorded by the library around their
                 launches, inside the timed region, on the launch stream) are the sub-object
                 `recurrent_kernels`.
--full adds, after the headline, the measurements that take runs of their own: the K steps repeated
(ms_per_step_repeats), the other arithmetics above, other_configs (cfg1, cfg3, cfg5 and the training-defaults
legs) and
  roofline_gemm— the dense products of a step at their real shapes, timed with events.
  cpu_baseline — oracle/cpu_baseline.py: the reference graph restated at TF op
                 granularity with PyTorch-CPU float32 ("port"), SURVEY.md 8(d)
                 protocol at full T, as a bounded sample (cfg2: 1 warm-up + median of 3 complete steps).  The reference's own
                 TF-1.8 trainer cannot run here.

--dump-outputs DIR writes what the LAST timed step of the headline region handed its caller
(before the repeats and the other legs train on) as DIR/<name>.npy: loss.npy (float32 [1]) and
params.npy (float32: the flat parameter buffer the step updated, or a fixed seeded sample of
DUMP_PARAMS elements of it when larger).  Inputs and initial weights are seeded, so two builds
run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, D, H, C = 32, 1000, 40, 512, 40
LAYER_T = (1000, 500, 250, 125)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
DUMP_LIMIT_BYTES = 64 * 10 ** 6
DUMP_PARAMS = 15 << 20         # --dump-outputs: parameters beyond this many are sampled (63 MB of float32, under the limit)
DUMP_SEED = 20240613           # ... with these fixed indices


def step_bytes(batch, hidden):
    """algorithmic bytes of ONE recurrent timestep of ONE direction"""
    return 4 * (hidden * 4 * hidden + batch * 4 * hidden + batch * 4 * hidden + 4 * batch * hidden)


CPU_CACHE = os.path.join(ROOT, 'gpurun_out', 'cpu_baseline_cache.json')


def cpu_baseline():
    """PyTorch-CPU float32 at TF op granularity (one [B,in+H]x[in+H,4H] matmul per
    frame per direction over the FULL T, autograd backward, per-variable clip + Adam), cfg1 and cfg2:
    cfg1: 2 warm-ups + median of 5 complete training steps; cfg2: 1 warm-up + median of 3 (a bounded sample).  Thread counts: 8(d) names "all physical
    cores"; for these small per-frame products that setting is an order of magnitude SLOWER than a
    handful of threads on a many-core host, so both are reported: `value` is cfg2 at the fastest
    thread count of a sweep on cfg1 (the CPU at its best), `all_physical_cores` holds cfg1 in full
    and cfg2 as far as its time bound allows."""
    from oracle import cpu_baseline as cb
    t_start = time.perf_counter()
    phys = cb.physical_cores()
    sweep = {}
    for n in sorted({t for t in (4, 8, 16, 32, 64, phys) if t <= phys}):
        sweep[n] = cb.time_config('cfg1', 1, 2, threads=n)['median_s']
        if len(sweep) >= 3 and sweep[n] > 1.5 * min(sweep.values()):
            break                                   # past the optimum: more threads only get slower
    cores = min(sweep, key=sweep.get)
    c1 = cb.time_config('cfg1', 2, 5, threads=cores)
    c1f = cb.time_config('cfg1', 2, 5, fused=True, threads=cores)
    # a BOUNDED sample (round 6: 1 warm-up + median of 3 complete steps, ~2.5 minutes; rounds 1-5 ran SURVEY 8(d)'s 2 + 5 and
    # spent 5 of the default run's 5.5 minutes here; a slower host stops after >= 2 steps once 3 minutes are used)
    c2 = cb.time_config('cfg2', 1, 3, threads=cores, budget_s=180.0)
    allc = {'cores': phys}
    if phys != cores:
        a1 = cb.time_config('cfg1', 2, 5, threads=phys, budget_s=60.0)
        allc['cfg1'] = {'value': a1['utt_per_s'], 'median_s': a1['median_s'], 'warmup': 2, 'steps': a1['steps_timed']}
        predicted = c2['median_s'] * a1['median_s'] / c1['median_s']
        if predicted < 60.0:
            a2 = cb.time_config('cfg2', 1, 2, threads=phys, budget_s=150.0)
            allc['cfg2'] = {'value': a2['utt_per_s'], 'median_s': a2['median_s'], 'warmup': 1, 'steps': a2['steps_timed']}
        else:
            allc['cfg2'] = {'value': round(32.0 / predicted, 4), 'median_s': round(predicted, 1), 'steps': 0,
                            'note': 'not run: predicted from cfg1 (cfg2 at the sweep optimum x cfg1 all-cores / cfg1 '
                                    'optimum); a measured step would exceed the bench budget'}
    else:
        allc['note'] = 'the sweep optimum IS all physical cores'
    # a cfg2 step at all physical cores MEASURED once outside this budget (python bench.py --cpu-all-cores), committed
    try:
        with open(os.path.join(ROOT, 'profiles', 'r04_cpu_all_cores.json')) as fid:
            m = json.load(fid)['cpu_all_physical_cores']
        if m['cores'] == phys:
            allc['cfg2_measured_once'] = {'value': m['value'], 'seconds_per_step': m['seconds_per_step'],
                                          'warmup': m['warmup'], 'steps': m['steps'],
                                          'source': 'profiles/r04_cpu_all_cores.json (bench.py --cpu-all-cores on a host '
                                                    'with the same core count; the in-budget figure above is an '
                                                    'extrapolation from cfg1 and overestimated the step 4.4 x there)'}
    except (OSError, ValueError, KeyError):
        pass
    out = {'value': c2['utt_per_s'], 'unit': 'utterances/sec', 'cores': cores, 'kind': 'port',
           'value_is': 'cfg2 at the best-of-sweep thread count (torch.set_num_threads(%d))' % cores,
           'sample': 'cfg2 (32 x 1000 x 40, 4x512 Listener + CTC), full T: %d warm-ups + median of %d complete '
                     'training steps (%s s each) of the reference graph restated at TF op granularity in '
                     'PyTorch-CPU float32 (per-frame [B,in+H]x[in+H,4H] matmul per direction, autograd, '
                     'per-variable clip+Adam); thread count = the fastest of a sweep on cfg1 '
                     '(seconds per step by thread count: %s; host has %d physical / %d logical cores); the '
                     'reference TF-1.8 trainer itself cannot run here'
                     % (c2['warmup'], c2['steps_timed'], c2['seconds_per_step'],
                        {k: round(v, 2) for k, v in sweep.items()}, phys, os.cpu_count()),
           'cfg1': {'value': c1['utt_per_s'], 'median_s': c1['median_s'], 'warmup': 2, 'steps': c1['steps_timed']},
           'all_physical_cores': allc,
           'upper_baseline_torch_nn_lstm': {
               'cfg1': {'value': c1f['utt_per_s'], 'median_s': c1f['median_s'], 'steps': c1f['steps_timed']},
               'note': 'same step with torch.nn.LSTM\'s fused CPU kernel on packed sequences instead of the '
                       'per-frame loop: faster than anything TF-1.8 dynamic_rnn could do'},
           'seconds_spent': round(time.perf_counter() - t_start, 1)}
    try:                                            # N > 1 lines of the same session carry this object
        os.makedirs(os.path.dirname(CPU_CACHE), exist_ok=True)
        with open(CPU_CACHE, 'w') as fid:
            json.dump({'host': socket.gethostname(), 'time': time.time(), 'cpu_baseline': out}, fid)
    except OSError:
        pass
    return out


CPU_COMMITTED = os.path.join(ROOT, 'profiles', 'cpu_baseline_last.json')


def cached_cpu_baseline(measure=True):
    """the cpu_baseline object of an N > 1 line — never null: (1) the N = 1 run's object of this host, if one was
    measured in the last day (the driver runs N = 1, 2, 4, 8 back to back); else (2) the last figure committed from an
    N = 1 run (profiles/cpu_baseline_last.json), labelled with the host it came from; else (3) ONE bounded measurement
    now on rank 0 (cfg2, 8 threads, one warm-up + one step: about a minute) — eight ranks never each run a baseline."""
    try:
        with open(CPU_CACHE) as fid:
            c = json.load(fid)
        if c['host'] == socket.gethostname() and time.time() - c['time'] < 86400:
            out = dict(c['cpu_baseline'])
            out['carried_from'] = 'the N=1 run on this host %.0f s earlier' % (time.time() - c['time'])
            return out
    except (OSError, ValueError, KeyError):
        pass
    try:
        with open(CPU_COMMITTED) as fid:
            c = json.load(fid)
        out = dict(c['cpu_baseline'])
        out['carried_from'] = ('profiles/cpu_baseline_last.json: the N=1 run of %s on host %s (%s); no N=1 run of this '
                               'host in the last day' % (c.get('commit', 'an earlier commit'), c.get('host', '?'),
                                                         c.get('date', '?')))
        return out
    except (OSError, ValueError, KeyError):
        pass
    if not measure:
        return None
    from oracle import cpu_baseline as cb
    c2 = cb.time_config('cfg2', 1, 1, threads=min(8, cb.physical_cores()))
    return {'value': c2['utt_per_s'], 'unit': 'utterances/sec', 'cores': min(8, cb.physical_cores()), 'kind': 'port',
            'sample': 'cfg2 (32 x 1000 x 40, 4x512 Listener + CTC), full T: 1 warm-up + 1 complete training step (%s s) of '
                      'the reference graph restated at TF op granularity in PyTorch-CPU float32, measured by rank 0 after '
                      'the timed region of this N > 1 run (no N=1 figure of this host or of the repository was found)'
                      % c2['seconds_per_step']}


def gemm_roofline(B, T, D, H, precision):
    """Second roofline object: the dense products of one cfg2 step (input projections, dz·Wxᵀ, xᵀ·dz,
    hᵀ·dz of every layer, both directions) launched back to back on the current stream and timed
    with events — MFMA-bound, fp32 peak from MI355X_MICROARCH.md."""
    import torch
    from nabu_amd import ops
    shapes = []
    Dl = D
    for l in range(4):
        BT = B * (T >> l)
        # the calls nabu_blstm_fwd / _bwd make, one set per direction (lstm.hip)
        shapes += [(0, 0, BT, 4 * H, Dl)] * 2                    # gates_d = x · Wx_d
        if l:
            shapes += [(0, 1, BT, Dl, 4 * H)] * 2                # dx (+)= dz_d · Wx_d^T
        shapes += [(1, 0, Dl, 4 * H, BT)] * 2 + [(1, 0, H, 4 * H, BT)] * 2     # dWx_d, dWh_d
        Dl = 4 * H
    bufs = {}
    def buf(n):
        if n not in bufs:
            bufs[n] = torch.randn(n, device='cuda')
        return bufs[n]
    calls = []
    for ta, tb, M, N, K in shapes:
        a = buf(M * K).view((K, M) if ta else (M, K))
        b = buf(K * N).view((N, K) if tb else (K, N))
        c = torch.empty((M, N), device='cuda')
        calls.append((a, b, c, bool(ta), bool(tb)))
    def run():
        for a, b, c, ta, tb in calls:
            ops.gemm(a, b, c, trans_a=ta, trans_b=tb, precision=precision)
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 3
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flops = sum(2.0 * M * N * K for _, _, M, N, K in shapes)
    tf = flops / ms / 1e9
    return {'bound': 'mfma', 'achieved': round(tf, 1), 'peak': 157.3, 'unit': 'TFLOP/s', 'frac': round(tf / 157.3, 4),
            'traffic': None, 'kernel': 'gemm_f32_fast_kernel<*> (+ split-K reduce)', 'ms_per_step': round(ms, 3),
            'flops_per_step': int(flops),
            'note': 'every dense product of a cfg2 step at its real shape, back to back, timed with events on the '
                    'launch stream; peak = dense fp32 MFMA (v_mfma_f32_32x32x2_f32) at 2.4 GHz'}


def gemm_roofline_pk(B, T, D, H, planes):
    """roofline_gemm for the packed bf16-plane products (gemm_pk.hip): the products nabu_blstm_fwd/_bwd launch for
    a cfg2 step at their real shapes (one launch fills both directions), back to back, timed with events; the
    pack kernels that convert their operands are timed separately.  `achieved` counts the MFMA work actually
    issued (6 plane products per fp32 product for planes = 3) against the dense bf16 peak."""
    import torch
    from nabu_amd import ops
    G = 4 * H
    prods, packs = [], []

    def operand(rows, K):
        src = torch.randn(rows, K, device='cuda')
        po = ops.PackedOperand(rows, K, planes, 'cuda')
        packs.append((po, src))
        return po
    Dl = D
    for l in range(4):
        BT = B * (T >> l)
        if Dl >= 256:
            prods.append((operand(BT, Dl), operand(2 * G, Dl), BT, 2 * G, 1))               # gates = x . [Wfw|Wbw]
            prods.append((operand(Dl, BT), operand(2 * G, BT), Dl, 2 * G, 1))               # dWx = x^T . dz
            prods.append((operand(BT, 2 * G), operand(Dl, 2 * G), BT, Dl, 1))               # dx = dz . Wx^T
        prods.append((operand(H, BT), operand(G, BT), H, G, 2))                             # dWh, both cells
        Dl = G
    for po, src in packs:
        ops.pk_pack(po, src)
    outs = [[torch.empty(M, N, device='cuda') for _ in range(nb)] for _, _, M, N, nb in prods]

    def run():
        for (a, b, M, N, nb), cs in zip(prods, outs):
            direct = 2 if planes == 2 else 0           # what nabu_blstm_fwd/_bwd ask for (include/nabu_hip.h)
            if nb == 1:
                ops.gemm_pk(a, b, cs[0], planes, direct=direct)
            else:
                ops.gemm_pk(a, b, None, planes, M=M, N=N, a_ptrs=[a.buf.data_ptr()] * 2, b_ptrs=[b.buf.data_ptr()] * 2, cs=cs,
                            direct=direct)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    ms = timed(run, 3)
    ms_pack = timed(lambda: [ops.pk_pack(po, src) for po, src in packs], 2)
    flops = sum(2.0 * M * N * a.K * nb for a, _, M, N, nb in prods)
    mult = {3: 6, 2: 3, 1: 1}[planes]
    tf = flops * mult / ms / 1e9
    return {'bound': 'mfma', 'achieved': round(tf, 1), 'peak': 2500.0, 'unit': 'TFLOP/s', 'frac': round(tf / 2500.0, 4),
            'traffic': None, 'kernel': 'gemm_pk_kernel<%d,*> (+ split-K reduce)' % planes, 'ms_per_step': round(ms, 3),
            'flops_per_step': int(flops), 'effective_fp32_tflops': round(flops / ms / 1e9, 1),
            'pack_ms_per_step': round(ms_pack, 3),
            'note': 'the packed-operand products of a cfg2 step at their real shapes, back to back, timed with events on '
                    'the launch stream; achieved = bf16 / fp16 MFMA flops issued (%d plane products per product) against the '
                    'dense bf16 (= fp16) peak of MI355X_MICROARCH.md; effective_fp32_tflops = 2MNK / time; pack_ms_per_step = '
                    'the fp32 -> plane conversions of the same operands (HBM-bound, not part of ms_per_step; planes = 2: '
                    'with the row-maximum pass)' % mult}


METRICS = {'cfg1': 'utterances/sec training step, 2x256 DBLSTM+CTC, batch 8x200x40 fbank',
           'cfg2': 'utterances/sec training step, 4x512 Listener+CTC, batch 32x1000x40 fbank',
           'cfg3': 'utterances/sec training step, Listener-512 + Speller (vanilla attention), batch 32x1000x40',
           'cfg5': 'utterances/sec training step, Listener-512 + Speller (location-aware attention), '
                   'bf16 input GEMMs, batch 64x1600x80'}
WORKLOADS = {'cfg1': 'cfg1: DBLSTM 2 x 256, DNNDecoder, CTC, Adam+clip; 8 utt x 200 frames x 40 fbank per GPU',
             'cfg2': 'cfg2: Listener 3 pyramidal + 1 BLSTM x512, DNNDecoder, CTC, Adam+clip; '
                     '32 utt x 1000 frames x 40 fbank per GPU',
             'cfg3': 'cfg3: cfg2 encoder + Speller (1x512 LSTMCell, Bahdanau attention), '
                     'average cross-entropy; 32 utt x 1000 frames x 40 fbank per GPU',
             'cfg5': 'cfg5: Listener-512 (bf16 input GEMMs) + Speller (location-aware attention); '
                     '64 utt x 1600 frames x 80 fbank per GPU'}
ALT_KEYS = {'f32': 'f32_products', 'bf16x6': 'alt_bf16x6', 'f16x3': 'alt_f16x3'}
# the other arithmetics the same step is timed under (object key of the line -> encoder cfg keys switched for the leg);
# `fp32_end_to_end`: exact-fp32 dense products AND the exact-fp32 recurrent kernels — float32 from the features to the
# update, as the reference's graph is (layer.py:35-47 on TF's fp32 MatMul)
ALT_LEGS = [('alt_bf16x6', {'gemm_precision': 'bf16x6'}),
            ('alt_f16x3', {'gemm_precision': 'f16x3'}),
            ('f32_products', {'gemm_precision': 'f32'}),
            ('fp32_end_to_end', {'gemm_precision': 'f32', 'recurrent_precision': 'f32'})]
REC_ARITH = {'default': 'recurrent product h.W_h: three fp16 plane products of row-scaled operands (fp32-equivalent, '
                        'lstm_persist_mxh.hip)',
             'f32': 'recurrent product h.W_h: exact fp32 (v_mfma_f32_4x4x1, lstm_persist.hip)'}
GEMM_ARITH = {'f32': 'f32 (v_mfma_f32_32x32x2_f32, exact fp32)',
              'bf16x6': 'fp32-equivalent on the bf16 matrix pipe: fp32 operands split exactly into 3 bf16 planes, 6 plane '
                        'products (v_mfma_f32_32x32x16_bf16), 16-k partial sums promoted to fp32 accumulators; error vs '
                        'float64 <= the exact-fp32 MFMA kernel\'s (tests/test_hip_gemm_pk.py)',
              'f16x3': 'fp32-equivalent on the fp16 matrix pipe: every operand row scaled by a power of two (row maximum '
                       'into [2^14, 2^15)) and held as two fp16 planes, 3 plane products (v_mfma_f32_32x32x16_f16) — chained '
                       'directly into the fp32 accumulators where that rounds less often than the exact-fp32 kernel does '
                       '(direct = 2: every product of this step), 16-k partial sums promoted otherwise; error vs float64 '
                       '0.51-0.66 x rms / 0.27-0.76 x max of the exact-fp32 MFMA kernel\'s on EVERY dense product of a '
                       'cfg2 step on the operands of a model trained for 50 updates, dz products included '
                       '(tests/test_hip_real_operands.py); the recipe ships this arithmetic '
                       '(config/recipes/cfg2_listener_ctc/model.cfg: gemm_precision)',
              'bf16x3': 'f32 operands split into 2 bf16 pieces, 3 bf16 MFMA products, f32 accumulate',
              'bf16': 'operands rounded to bf16, f32 accumulate'}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--mode', default='auto', choices=['auto', 'stepwise', 'persistent'])
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-alt', action='store_true',
                    help='skip the measurements of the same step with the other fp32-class arithmetics of the dense products')
    ap.add_argument('--no-gemm-roofline', action='store_true',
                    help='skip the roofline_gemm measurement (keeps a kernel trace of this command to the training steps)')
    ap.add_argument('--gemm-precision', default=None, choices=['f32', 'bf16x6', 'f16x3', 'bf16x3', 'bf16'],
                    help='arithmetic of the BLSTM layers\' dense products (include/nabu_hip.h).  Default: what the '
                         'workload\'s RECIPE ships (cfg2: f16x3 = fp32-equivalent three-plane products of row-scaled '
                         'fp16 operands); given, it overrides the recipe\'s encoder.gemm_precision key for this run '
                         '(bf16x6 = fp32-equivalent six-plane products on the bf16 matrix pipe, f32 = exact fp32 '
                         'MFMA).  The line names the arithmetic in config.gemm_arith and, with --full, carries the other '
                         'two, timed with the same steps / warm-up, as `f32_products` / `alt_bf16x6` / `alt_f16x3`, plus '
                         '`fp32_end_to_end` (exact-fp32 products AND recurrence)')
    ap.add_argument('--workload', default='cfg2', choices=['cfg1', 'cfg2', 'cfg3', 'cfg5'],
                    help='cfg2 (default) is the BASELINE.json metric; cfg3 = same encoder + Speller; cfg5 = '
                         'location-aware LAS, batch 64x1600x80, bf16 input GEMMs (BASELINE.json configs[2]/[4]), '
                         'for information')
    ap.add_argument('--dry-run', action='store_true',
                    help='first-contact check of the multi-rank path: start / join the ranks exactly as a measurement '
                         'would (self-launch or the given environment, rendezvous over 127.0.0.1, device assignment), '
                         'run one collective, print one JSON line and stop before the workload.  With fewer visible '
                         'GPUs than ranks the process group is gloo and the ranks share the devices round-robin.')
    ap.add_argument('--cpu-all-cores', action='store_true',
                    help='ONLY measure one cfg2 training step of the CPU port at ALL physical cores of this host (SURVEY.md '
                         '8(d) names that setting; it takes ~10 minutes on a 128-core host, which is why the --full run '
                         'reports it as a labelled prediction) and print it as one JSON line; no GPU work')
    ap.add_argument('--shrink', action='store_true',
                    help='NOT a measurement: cfg2\'s recipe at 4 utterances x 64 frames, 64 units — lets the tests run the '
                         'whole multi-rank line (ranks, exchange, carried cpu_baseline, roofline object) in seconds; the '
                         'line says config.shrunk = true')
    ap.add_argument('--training-defaults', action='store_true',
                    help='NOT the headline: the workload with the REFERENCE\'s regularisation defaults switched on — Listener '
                         'input_noise 0.6 and dropout keep 0.5 (ed_encoders/defaults/listener.cfg), Speller output dropout keep '
                         '0.5 and sample_prob 0.1 (ed_decoders/defaults/speller.cfg) — instead of the deterministic settings '
                         'the parity configs of SURVEY.md 8(d) prescribe; the line says config.training_defaults = true')
    ap.add_argument('--full', action='store_true',
                    help='measure everything beyond the headline after it: the K timed steps repeated (--repeats, default '
                         '3 here), the other arithmetics of the dense products (alt legs), roofline_gemm, the other '
                         'single-GPU configs (other_configs) and the CPU baseline; the --no-* options skip single legs.  '
                         'Without it a run sets up, warms up, times the K steps, dumps its outputs if asked to and prints '
                         'the line')
    ap.add_argument('--repeats', type=int, default=None,
                    help='the K timed steps are repeated this many times inside the same command (same bracket each time); '
                         'default 3 with --full, else 1.  The headline value is the FIRST region — warm-up W, then exactly K '
                         'steps — the line carries all of them as ms_per_step_repeats with their spread, and the shader '
                         'clock the recurrent kernels ran at (effective_clock), so that a slow box of the pool is visible '
                         'as such')
    ap.add_argument('--no-other-configs', action='store_true',
                    help='skip the other single-GPU BASELINE.json configs (cfg1, cfg3, cfg5\'s per-GPU share) and the '
                         'training-defaults legs that the --full N = 1 cfg2 run times after the headline (other_configs)')
    ap.add_argument('--other-steps', type=int, default=10, help='timed steps of every other_configs leg (3 warm-up steps each)')
    ap.add_argument('--allreduce', default='flat', choices=['flat', 'bucketed', 'both'],
                    help='gradient exchange of the data-parallel mode (trainer cfg key allreduce_buckets).  both: the '
                         'headline is timed with the flat exchange, then the same steps once more with the bucketed one '
                         '(ranks.allreduce_both) — one run answers which of the two the scaling curve should use')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step of the headline region returned to its '
                         'caller as DIR/<name>.npy (rank 0): loss.npy and params.npy, float32; parameters beyond '
                         'DUMP_PARAMS elements are a fixed, seeded sample.  The line lists the files as outputs_dumped')
    args = ap.parse_args(argv)
    if not args.full:
        args.no_cpu_baseline = args.no_alt = args.no_gemm_roofline = args.no_other_configs = True
    if args.repeats is None:
        args.repeats = 3 if args.full else 1
    return args


def sample_flat(n):
    """the indices params.npy holds of a flat buffer of n elements: all of them, or DUMP_PARAMS fixed, seeded ones"""
    import numpy as np
    if n <= DUMP_PARAMS:
        return None
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_PARAMS, replace=False))


def dump_outputs(directory, arrays):
    """write {name: array} as directory/<name>.npy (float32 / float64 only, DUMP_LIMIT_BYTES in all); returns
    {name: shape} for the line"""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit('bench.py: --dump-outputs would write %d bytes (limit %d)' % (total, DUMP_LIMIT_BYTES))
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise SystemExit('bench.py: --dump-outputs %s is %s, not float32 / float64' % (name, a.dtype))
        np.save(os.path.join(directory, name + '.npy'), a)
    return {name: list(a.shape) for name, a in arrays.items()}


# ------------------------------------------------------------------ launching the ranks
def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_command(argv, nproc, script=None, port=None):
    """the command that runs `script argv` as nproc ranks on this node (one process per GPU)"""
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc),
            '--master-addr', '127.0.0.1', '--master-port', str(port or free_port()),
            script or os.path.abspath(__file__)] + list(argv)


def self_launch(argv, nproc, script=None):
    """`python bench.py --gpus N` without ranks in the environment: start them (the local
    'cluster' of the reference's single_machine mode).  Rank 0's JSON line reaches our stdout
    through the inherited descriptors.  Returns the launcher's exit code."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')       # dmabuf IPC for RCCL on this driver
    env.setdefault('OMP_NUM_THREADS', '4')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    return subprocess.call(launch_command(argv, nproc, script), env=env)


def make_server():
    from nabu_amd.computing import dist
    return dist.create_server()


def dry_run(args):
    """everything a measurement does up to and including init_process_group + one collective"""
    import torch
    from nabu_amd.computing import dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    ngpu = torch.cuda.device_count() if torch.cuda.is_available() else 0
    shared = dist.ranks_share_devices(world, ngpu) or (world > 1 and ngpu == 0)
    if shared and ngpu:
        os.environ['LOCAL_RANK'] = str(int(os.environ.get('LOCAL_RANK', '0')) % ngpu)
    server = dist.create_server(backend='gloo' if shared else None)
    dev = torch.device('cuda', torch.cuda.current_device()) if ngpu else torch.device('cpu')
    t = torch.full((4,), float(server.rank + 1), device='cpu' if server.backend == 'gloo' else dev)
    server.all_reduce_sum_(t)
    expect = world * (world + 1) / 2.0
    ok = bool((t == expect).all().item())
    server.barrier()
    if server.rank == 0:
        print(json.dumps({'dry_run': True, 'ok': ok, 'world_size_seen': server.world_size, 'backend': server.backend,
                          'visible_gpus': ngpu, 'ranks_share_devices': shared, 'all_reduce_sum': float(t[0].item()),
                          'master': '%s:%s' % (os.environ.get('MASTER_ADDR'), os.environ.get('MASTER_PORT'))}), flush=True)
    server.shutdown()
    return 0 if ok else 1


# ------------------------------------------------------------------ the workload on the GPU
class HipWorkload(object):
    """the BASELINE workload on this rank's GPU through the recipe API"""

    def __init__(self, args, server):
        import torch
        from nabu_amd import recipes, ops, _hip
        from nabu_amd.neuralnetworks.components import layer
        from nabu_amd.neuralnetworks.trainers import trainer_factory
        from nabu_amd.processing.synthetic import SyntheticData
        if not torch.cuda.is_available():
            raise SystemExit('bench.py needs a GPU (the HIP path has no CPU fallback)')
        if server.world_size == 1:
            torch.cuda.set_device(0)
        self.torch, self.ops, self._hip, self.layer = torch, ops, _hip, layer
        self.args, self.server = args, server
        rank = server.rank
        _hip.lib()
        self.shared = bool(getattr(server, 'shared_devices', False))
        if self.shared:
            # more ranks than GPUs (first-contact runs, tests): the ranks' launches interleave on one device, and the
            # persistent recurrent kernels need a whole device to themselves -> one launch per frame
            args.mode = 'stepwise'
        layer.LSTM_MODE[0] = {'auto': ops.LSTM_AUTO, 'stepwise': ops.LSTM_STEPWISE,
                              'persistent': ops.LSTM_PERSISTENT}[args.mode]
        self.B, self.T, self.D, self.H = B, T, D, H
        self.layer_t = None
        over = {'trainer.allreduce_buckets': 'True' if args.allreduce == 'bucketed' else 'False'}   # (both: flat first)
        if args.gemm_precision:          # otherwise: the arithmetic the recipe ships
            over['encoder.gemm_precision'] = args.gemm_precision
        if getattr(args, 'training_defaults', False):
            over.update({'encoder.input_noise': '0.6', 'encoder.dropout': '0.5'})
            if args.workload in ('cfg3', 'cfg5'):
                over.update({'decoder.dropout': '0.5', 'decoder.sample_prob': '0.1'})
        if args.workload == 'cfg1':
            # BASELINE.json configs[0]: DBLSTM 2 x 256 + CTC, 8 x 200 x 40 (the reference's CPU-runnable case)
            self.B, self.T, self.D, self.H = 8, 200, 40, 256
            self.layer_t = [200, 200]
            mc, tc, ec = recipes.load_recipe('cfg1_dblstm_ctc', **over)
            data = SyntheticData(8, 200, 40, min_frames=200, min_labels=10, max_labels=40, seed=1234 + rank)
        elif args.workload == 'cfg5':
            self.B, self.T, self.D = 64, 1600, 80
            mc, tc, ec = recipes.load_recipe('cfg5_las_location', **over)
            data = SyntheticData(64, 1600, 80, min_frames=1600, min_labels=40, max_labels=159, eos=True,
                                 time_reduction=8, seed=5234 + rank)
        elif args.workload == 'cfg3':
            mc, tc, ec = recipes.load_recipe('cfg3_las_vanilla', **over)
            data = SyntheticData(B, T, D, min_frames=T, min_labels=20, max_labels=79, eos=True, time_reduction=8,
                                 seed=3234 + rank)
        elif args.shrink:
            self.B, self.T, self.H = 4, 64, 64
            over.update({'encoder.num_units': '64', 'trainer.batch_size': '4'})
            mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
            data = SyntheticData(4, 64, D, min_frames=64, min_labels=2, max_labels=5, time_reduction=8, seed=4234 + rank)
        else:
            mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
            data = SyntheticData(B, T, D, min_frames=T, min_labels=20, max_labels=60, time_reduction=8,
                                 seed=4234 + rank)
        if self.layer_t is None:
            self.layer_t = [self.T >> i for i in range(4)]
        self.tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec,
                                                      expdir=None, server=server, task_index=rank)
        self.tr.time_allreduce = server.world_size > 1
        if server.world_size > 1 and args.allreduce == 'bucketed':
            self.tr.schedule_log = []
        # the arithmetic of the BLSTM layers' dense products this run computes in: the recipe's, unless overridden
        self.precision = mc.get('encoder', 'gemm_precision') if mc.has_option('encoder', 'gemm_precision') else 'f32'
        self.batches = [self.tr.to_device(data.batch(i)) for i in range(2)]      # resident in HBM
        # the event profiler is armed during the warm-up as well: its first use (event pool creation
        # inside the HIP runtime) stalls the queue for tens of milliseconds once
        self.prof = ops.enable_profiler()
        self.timing = False
        self.loss = None

    units_per_step = property(lambda self: self.B)

    # HIP events around the recurrent launches cost the stream ~6 us each (a queue barrier per record: 16 per cfg2
    # step): every PROFILE_EVERY-th step of the timed region carries them — counted from its THIRD step, whose first
    # launch does not follow the idle bracket in front of the region — the others run as a user's step does
    PROFILE_EVERY = 16

    def profiled(self, i):
        return (i - min(2, self.args.steps - 1)) % self.PROFILE_EVERY == 0

    def step(self, i):
        if self.timing:
            self.prof.enabled = self.profiled(i)
            # the same steps also bracket the decoder's two calls (recipes with a Speller) with events on the launch stream
            from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
            rnn_decoder.dynamic_decode.events = self.dec_events if self.prof.enabled else None
        self.loss = self.tr.step(self.batches[i % 2])

    def sync(self):
        self.torch.cuda.synchronize()

    def check(self):
        from nabu_amd.neuralnetworks.trainers import loss_functions
        loss_functions.check_status()
        self.ops.check_persist_status()

    def start_timed_region(self):
        self.prof.collect()                                         # drop the warm-up records
        self.tr.allreduce_ms = []
        self.dec_events = []
        self.timing = True

    def end_timed_region(self):
        from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
        rnn_decoder.dynamic_decode.events = None
        self.timing = False
        self.prof.enabled = False
        self.recs = self.prof.collect()
        self.final_loss = float(self.loss.item())

    def outputs(self):
        """what the last step returned to its caller, copied to the host: the loss and the parameters it updated"""
        import numpy as np
        flat = self.tr.model.store.flat
        idx = sample_flat(flat.numel())
        if idx is not None:
            flat = flat[self.torch.from_numpy(idx).to(flat.device)]
        return {'loss': self.loss.detach().float().cpu().numpy().reshape(-1).astype(np.float32),
                'params': flat.detach().cpu().numpy().astype(np.float32)}

    def reduce_max(self, values):
        t = self.torch.tensor(values, dtype=self.torch.float64, device='cuda')
        if self.server.world_size > 1:
            self.torch.distributed.all_reduce(t, op=self.torch.distributed.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def gather(self, value):
        t = self.torch.tensor([value], dtype=self.torch.float64, device='cuda')
        if self.server.world_size == 1:
            return [float(value)]
        out = [self.torch.zeros_like(t) for _ in range(self.server.world_size)]
        self.torch.distributed.all_gather(out, t)
        return [float(o.item()) for o in out]

    def gather_i64(self, value):
        t = self.torch.tensor([int(value)], dtype=self.torch.int64, device='cuda')
        if self.server.world_size == 1:
            return [int(value)]
        if self.server.backend == 'gloo':
            t = t.cpu()
        out = [self.torch.zeros_like(t) for _ in range(self.server.world_size)]
        self.torch.distributed.all_gather(out, t)
        return [int(o.item()) for o in out]

    def weights_checksum(self):
        '''order-independent, bit-exact fingerprint of this replica's parameters: the int64 sum of the flat fp32 buffer's
        bit patterns (measurement code: torch arithmetic is fine here, the product path has none)'''
        flat = self.tr.model.store.flat
        return int(flat.view(self.torch.int32).to(self.torch.int64).sum().item())

    def replicas_identical(self, when):
        '''collective: every rank's weights checksum; raises on every rank when they differ (a silent replica drift would
        otherwise read as a loss difference).  Returns the entry for the line's `ranks` object.'''
        sums = self.gather_i64(self.weights_checksum())
        same = len(set(sums)) == 1
        if not same:
            raise SystemExit('bench.py: the replicas hold DIFFERENT weights %s the timed region: checksums %s'
                             % (when, ['%016x' % (v & 0xFFFFFFFFFFFFFFFF) for v in sums]))
        return {'identical': True, 'checksum': '%016x' % (sums[0] & 0xFFFFFFFFFFFFFFFF)}

    def effective_clock(self):
        '''GHz the chip sustained under the last recurrent launches (ops.persist_clocks: in-kernel clock stamps)'''
        try:
            return self.ops.persist_clocks()
        except Exception as exc:          # noqa: BLE001 — a diagnostic must not take the line down
            return {'error': str(exc)}

    def allreduce_ms_per_step(self):
        ev = getattr(self.tr, 'allreduce_ms', [])
        if not ev:
            return None
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev)

    def set_allreduce(self, kind):
        '''switch the trainer's gradient exchange between measurements (--allreduce both)'''
        tr = self.tr
        tr.buckets = tr._make_buckets() if (kind == 'bucketed' and self.server.world_size > 1) else None
        tr.schedule_log = [] if tr.buckets is not None else None
        tr.allreduce_ms = []

    def rank_paths(self):
        '''(recurrence persistent?, decoder persistent?) of THIS rank: 1 / 0, decoder -1 when the model has none'''
        import ctypes
        _hip, layer = self._hip, self.layer
        desc = _hip.BlstmDesc(ctypes.sizeof(_hip.BlstmDesc), self.B, self.T, self.D, self.H, self.T, layer.LSTM_MODE[0], 0)
        rec = int(bool(_hip.lib().nabu_blstm_uses_persistent(ctypes.byref(desc))))
        dec = -1
        from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
        last = getattr(rnn_decoder.dynamic_decode, 'last_paths', None)      # (forward, backward) of the last decode call
        if last is not None:
            dec = int(bool(last[0])) + 2 * int(bool(last[1]))               # bit 0 forward, bit 1 backward persistent
        return rec, dec

    def bucket_schedule(self):
        """bucketed exchange: (bucket, 'hook' = between a recurrence and the products behind it / after the deferred
        weight gradients, 'final' = at the optimiser) of the last step, in launch order"""
        log = getattr(self.tr, 'schedule_log', None)
        if not log:
            return None
        n = len(self.tr.buckets)
        return [list(e) for e in log[-n:]]

    def alt(self, steps):
        """the same step under the other fp32-class arithmetics: [(line key, cfg keys, seconds, loss)]"""
        if self.precision not in ALT_KEYS or self.args.workload != 'cfg2' or self.args.no_alt:
            return []
        return [(key, conf) + alt_gemm_arith(self.tr, self.batches, self.server, steps, max(self.args.warmup, 1), conf)
                for key, conf in ALT_LEGS if conf != {'gemm_precision': self.precision}]

    def describe(self, dt):
        """workload-specific part of the JSON line (rank 0)"""
        import ctypes
        args, _hip, layer = self.args, self._hip, self.layer
        B_, T_, D_, H_ = self.B, self.T, self.D, self.H
        # roofline of the dominant kernel: recurrent step(s), per launch
        desc = _hip.BlstmDesc(ctypes.sizeof(_hip.BlstmDesc), B_, T_, D_, H_, T_, layer.LSTM_MODE[0], 0)
        persistent = bool(_hip.lib().nabu_blstm_uses_persistent(ctypes.byref(desc)))
        recs = self.recs
        tot_ms = sum(r[4] for r in recs)
        tot_steps = sum(r[2] for r in recs)                   # timesteps covered (both directions each)
        tot_bytes = sum(2 * r[2] * step_bytes(r[1], r[3]) for r in recs)
        prof_steps = max(len([i for i in range(args.steps) if self.profiled(i)]), 1)
        launches = len(recs) if persistent else tot_steps
        per_launch_bytes = tot_bytes / max(launches, 1)
        per_launch_s = tot_ms * 1e-3 / max(launches, 1)
        achieved = per_launch_bytes / per_launch_s / 1e9 if per_launch_s > 0 else 0.0
        # HBM traffic per launch of the same kernels from the PMC passes (rocprofv3 --pmc FETCH_SIZE /
        # WRITE_SIZE, separate runs of this command; summarised by tools/pmc_summary.py with the
        # gfx950 corrections of MI355X_MICROARCH.md).  null when this workload was not profiled.
        traffic = None
        for name in ('r06_cfg2_pmc_traffic.json', 'r05_cfg2_pmc_traffic.json', 'r04b_cfg2_pmc_traffic.json', 'r04_cfg2_pmc_traffic.json', 'r03_cfg2_pmc_traffic.json'):
            pmc = os.path.join(ROOT, 'profiles', name)
            if persistent and args.workload == 'cfg2' and os.path.exists(pmc):
                with open(pmc) as fid:
                    traffic = int(json.load(fid)['lstm_persist_traffic_bytes_per_launch'])
                break
        step_bytes_total = 2 * 2 * sum(self.layer_t) * step_bytes(B_, H_)
        step_s = dt / args.steps
        frac_step = step_bytes_total / step_s / (HBM_PEAK_GBS * 1e9)
        kname = ('lstm_mxh_{fwd,bwd}_kernel (lstm_mxf_* for 33-64 rows; lstm_persist_* where the fp16-plane kernels do not apply or are switched off)'
                 if persistent else 'lstm_step_{fwd,bwd}_kernel')
        roofline = {'bound': 'hbm', 'achieved': round(step_bytes_total / step_s / 1e9, 1), 'peak': HBM_PEAK_GBS,
                    'unit': 'GB/s', 'frac': round(frac_step, 4), 'traffic': traffic, 'kernel': kname,
                    'bytes_per_step': int(step_bytes_total), 'launches_per_step': launches // prof_steps,
                    'recurrent_kernels': {
                        'achieved': round(achieved, 1), 'frac': round(achieved / HBM_PEAK_GBS, 4),
                        'bytes_per_launch': int(per_launch_bytes), 'us_per_launch': round(per_launch_s * 1e6, 3),
                        'launches_timed': launches, 'steps_with_events': prof_steps, 'ms_per_step': round(tot_ms / prof_steps, 3),
                        'us_per_sequential_step': round(tot_ms * 1e3 / max(tot_steps, 1), 3)},
                    'note': 'SURVEY.md 8(d): algorithmic bytes of the recurrent LSTM steps of ONE training step (W_h '
                            'streamed per timestep model) over the measured step time — the step also pays for its '
                            'MFMA-bound dense products, so this is the whole-step figure the 0.40 target is stated on; '
                            'recurrent_kernels = the same bytes per launch over the launch duration from HIP events the '
                            'library records around the recurrent launches of every 16th step of the timed region, from its third (an '
                            'event record is a queue barrier, ~6 us: 16 of them per step would be paid by the metric); '
                            'traffic = HBM bytes '
                            'per recurrent launch from the rocprofv3 PMC passes under profiles/'}
        return {
            'metric': METRICS[args.workload],
            'dtype': ('f32' if self.precision == 'f32' else 'f32 (%s products)' % self.precision if self.precision in ALT_KEYS
                      else 'f32 state / %s products' % self.precision),
            'config': {'workload': WORKLOADS[args.workload], 'frames': T_,
                       'recurrent_path': 'persistent' if persistent else 'stepwise',
                       'gemm_arith': GEMM_ARITH[self.precision],
                       'gemm_precision_from': 'command line' if args.gemm_precision else 'recipe (encoder.gemm_precision)',
                       'shrunk': bool(getattr(args, 'shrink', False)),
                       'training_defaults': bool(getattr(args, 'training_defaults', False))},
            'roofline': roofline,
            'roofline_gemm': (None if args.workload != 'cfg2' or args.no_gemm_roofline
                              else gemm_roofline(B_, T_, D_, H_, self.precision) if self.precision == 'f32'
                              else gemm_roofline_pk(B_, T_, D_, H_, 3) if self.precision == 'bf16x6'
                              else gemm_roofline_pk(B_, T_, D_, H_, 2) if self.precision == 'f16x3' else None),
            'final_loss': round(self.final_loss, 4),
            'roofline_decoder': self.roofline_decoder(),
        }

    def roofline_decoder(self):
        '''The attention decoder against ITS roofline (recipes with a Speller; null otherwise): a decoder step reads the
        keys [Te, U] and the values [Te, E] of every utterance once per pass — algorithmic bytes of the two calls
        (nabu_speller_fwd / _bwd: all L steps each) over their duration from events on the launch stream (the step
        chain's four streams fork from and join it inside the calls), every PROFILE_EVERY-th step of the timed region.'''
        ev = getattr(self, 'dec_events', None)
        if not ev:
            return None
        out = {'bound': 'hbm', 'peak': HBM_PEAK_GBS, 'unit': 'GB/s'}
        tot_b = tot_ms = 0.0
        for name in ('fwd', 'bwd'):
            recs = [(sh, a.elapsed_time(b)) for kind, sh, a, b in ev if kind == name]
            if not recs:
                continue
            sh = recs[0][0]
            nbytes = 4.0 * sh['L'] * sh['B'] * sh['Te'] * (sh['U'] + sh['E'])
            ms = sum(t for _, t in recs) / len(recs)
            out[name] = {'ms_per_call': round(ms, 3), 'us_per_decoder_step': round(ms * 1e3 / sh['L'], 2),
                         'achieved': round(nbytes / (ms * 1e-3) / 1e9, 1), 'frac': round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            tot_b += nbytes
            tot_ms += ms
        sh = ev[0][1]
        out.update({'achieved': round(tot_b / (tot_ms * 1e-3) / 1e9, 1), 'frac': round(tot_b / (tot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    'ms_per_step': round(tot_ms, 3), 'decoder_steps': sh['L'], 'utterances': sh['B'], 'frames': sh['Te'],
                    'bytes_per_decoder_step_and_pass': int(4 * sh['B'] * sh['Te'] * (sh['U'] + sh['E'])),
                    'calls_timed': len(ev),
                    'note': 'keys [Te, U] + values [Te, E] of every utterance read once per decoder step and pass (SURVEY.md 8(d): '
                            '(U+E)·Te·4 bytes per utterance and step) over the wall time of the two decoder calls; the persistent '
                            'decoder (cfg3) keeps its slices of both in LDS for the whole call, so its HBM traffic is far below '
                            'this figure — the fraction prices the step loop, not the memory system'})
        return out

    def wants_cpu_baseline(self):
        return self.args.workload == 'cfg2'


def make_workload(args, server):
    return HipWorkload(args, server)


# ------------------------------------------------------------------ the protocol
def run(args, server, wl):
    """W untimed warm-up steps, then EXACTLY K steps bracketed by device sync + barrier on both
    sides; the time is the MAX over ranks; rank 0 returns the JSON object (others None)."""
    rank, world = server.rank, server.world_size
    replica = {}
    # bit-identical replicas: checked behind the FIRST warm-up step (a 135 MB checksum pass right in front of the timed
    # region would flush the caches the steps run out of: the first region then ran 0.5-1 % slower than its repeats) and
    # after the last step of the command; a single process has nothing to compare with before it has trained
    for i in range(max(args.warmup, 1)):
        wl.step(i)
        if i == 0 and world > 1 and hasattr(wl, 'replicas_identical'):     # (the first step builds the flat parameter buffer)
            replica['before_timed_region'] = wl.replicas_identical('before')
    wl.check()
    wl.sync()
    wl.start_timed_region()
    server.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        wl.step(i)
    wl.sync()
    server.barrier()
    dt_rank = time.perf_counter() - t0
    wl.end_timed_region()
    wl.check()
    # taken now: the repeats and the other legs below go on training the same weights
    dumped = wl.outputs() if getattr(args, 'dump_outputs', None) and rank == 0 else None
    clocks = wl.effective_clock() if hasattr(wl, 'effective_clock') else None
    # the same K steps again (same bracket), repeats - 1 times: the headline stays the first region
    dt_repeats = []
    for _ in range(max(getattr(args, 'repeats', 1), 1) - 1):
        wl.sync()
        server.barrier()
        t1 = time.perf_counter()
        for i in range(args.steps):
            wl.step(i)
        wl.sync()
        server.barrier()
        dt_repeats.append(time.perf_counter() - t1)
    if dt_repeats:
        wl.check()
    if hasattr(wl, 'replicas_identical'):
        replica['after_timed_region'] = wl.replicas_identical('after')
    ar_ms = wl.allreduce_ms_per_step()
    ar_ranks = wl.gather(ar_ms if ar_ms is not None else 0.0)
    both = None
    if getattr(args, 'allreduce', 'flat') == 'both' and world > 1:
        # the same steps once more with the bucketed exchange: same protocol, not the headline
        wl.set_allreduce('bucketed')
        for i in range(max(args.warmup, 1)):
            wl.step(i)
        wl.sync()
        server.barrier()
        t1 = time.perf_counter()
        for i in range(args.steps):
            wl.step(i)
        wl.sync()
        server.barrier()
        dt_b = wl.reduce_max([time.perf_counter() - t1])[0]
        wl.check()
        ar_b = wl.allreduce_ms_per_step()
        ar_b_ranks = wl.gather(ar_b if ar_b is not None else 0.0)
        both = {'flat': None, 'bucketed': {'ms_per_step': round(dt_b / args.steps * 1e3, 3),
                                            'value': round(world * wl.units_per_step * args.steps / dt_b, 2),
                                            'exposed_allreduce_ms_per_step': [round(v, 3) for v in ar_b_ranks],
                                            'bucket_schedule_last_step': wl.bucket_schedule()}}
        wl.set_allreduce('flat')
    alt = wl.alt(args.steps)
    red = wl.reduce_max([dt_rank] + [a[2] for a in alt] + dt_repeats)
    rep = [red[0]] + red[1 + len(alt):]
    red = red[:1 + len(alt)]
    per_rank = wl.gather(dt_rank)
    paths = wl.rank_paths() if hasattr(wl, 'rank_paths') else (-1, -1)
    rec_ranks, dec_ranks = wl.gather(paths[0]), wl.gather(paths[1])
    dt = red[0]
    if rank != 0:
        return None
    out = {'metric': None, 'value': round(world * wl.units_per_step * args.steps / dt, 2), 'unit': 'utterances/sec',
           'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
           'ms_per_step': round(dt / args.steps * 1e3, 3), 'higher_is_better': True, 'scaling': 'weak',
           'vs_baseline': None, 'dtype': None, 'data': 'synthetic'}
    rep_ms = [round(t / args.steps * 1e3, 3) for t in rep]
    out['ms_per_step_repeats'] = rep_ms
    out['repeats'] = {'n': len(rep_ms), 'steps_each': args.steps, 'median_ms_per_step': sorted(rep_ms)[len(rep_ms) // 2],
                      'min_ms_per_step': min(rep_ms), 'max_ms_per_step': max(rep_ms),
                      'spread': round((max(rep_ms) - min(rep_ms)) / min(rep_ms), 4),
                      'note': 'the K timed steps repeated inside the same command, same barrier + sync bracket, MAX over '
                              'ranks each; ms_per_step / value are the FIRST region (W warm-up steps, then exactly K steps)'}
    out['effective_clock'] = None if clocks is None else {
        'recurrent_fwd_ghz': clocks.get('fwd'), 'recurrent_bwd_ghz': clocks.get('bwd'), 'spec_max_ghz': 2.4,
        'note': 'shader cycles (s_memtime) over wall time (100 MHz counter) between the first and the last instruction of '
                'the LAST fp16-plane recurrent launch of each pass in the headline region, stamped by the kernels '
                'themselves (lstm_persist_dev.h, clock_stamp): the clock the chip sustained under the latency-bound '
                'kernels — boxes of the pool differ by a few per cent here'}
    out.update(wl.describe(dt))
    out['config'].update({'global_batch': world * wl.units_per_step, 'parallelism': 'dp%d' % world})
    out['ranks'] = {'world_size_seen': world, 'backend': server.backend,
                    'ms_per_step_per_rank': [round(t / args.steps * 1e3, 3) for t in per_rank],
                    'allreduce': ('flat' if getattr(args, 'allreduce', 'flat') == 'both' else getattr(args, 'allreduce', 'flat'))
                                 if world > 1 else None,
                    'allreduce_ms_per_step': [round(v, 3) for v in ar_ranks] if world > 1 else None,
                    'ranks_share_devices': bool(getattr(server, 'shared_devices', False)),
                    # which path every rank ran: a rank that fell to the step-wise recurrence (occupancy check, a
                    # partitioned device) or the decoder's step chain shows here, not only as a slow rank
                    'recurrence_persistent_per_rank': [int(v) for v in rec_ranks],
                    'decoder_persistent_per_rank': [int(v) for v in dec_ranks],
                    'bucket_schedule_last_step': wl.bucket_schedule(),
                    # bit-identical replicas, asserted (all-gather of a checksum of the flat parameter buffer) before the
                    # timed region and after its last step: a drift would otherwise read as a loss difference
                    'replica_weights': replica or None,
                    'collective_library': collective_library_info(server) if world > 1 else None}
    if both is not None:
        both['flat'] = {'ms_per_step': out['ms_per_step'], 'value': out['value'],
                        'exposed_allreduce_ms_per_step': out['ranks']['allreduce_ms_per_step']}
        out['ranks']['allreduce_both'] = both
    for i, (key, conf, _, alt_loss) in enumerate(alt):
        n = args.steps
        step_bytes_total = 2 * 2 * sum(wl.layer_t) * step_bytes(wl.B, wl.H)
        out[key] = {
            'note': 'the identical step (same weights stream, batches and protocol as the headline: %d warm-up steps, %d '
                    'timed steps, barrier + sync bracket, MAX over ranks) in another arithmetic; '
                    'not the headline value' % (max(args.warmup, 1), n),
            'gemm_arith': GEMM_ARITH[conf['gemm_precision']],
            'recurrent_arith': REC_ARITH[conf.get('recurrent_precision', 'default')],
            'value': round(world * wl.units_per_step * n / red[1 + i], 2), 'ms_per_step': round(red[1 + i] / n * 1e3, 3),
            'steps': n, 'final_loss': round(alt_loss, 4),
            'roofline_frac': round(step_bytes_total / (red[1 + i] / n) / (HBM_PEAK_GBS * 1e9), 4)}
    if (world == 1 and getattr(args, 'workload', None) == 'cfg2' and not getattr(args, 'no_other_configs', True)
            and not getattr(args, 'shrink', False) and not getattr(args, 'training_defaults', False)
            and isinstance(wl, HipWorkload)):
        out['other_configs'] = other_configs(args, server)
    if not args.no_cpu_baseline and wl.wants_cpu_baseline():
        out['cpu_baseline'] = cpu_baseline() if world == 1 else cached_cpu_baseline()
    if dumped is not None:
        out['outputs_dumped'] = dump_outputs(args.dump_outputs, dumped)

    return out


def collective_library_info(server):
    '''what the SCALE line needs to explain itself: the collective library's version, the environment switches that
    steer it, and the xGMI links the topology files of this node show'''
    info = {'backend': server.backend}
    try:
        import torch
        if server.backend == 'nccl':
            info['rccl_version'] = '.'.join(str(v) for v in torch.cuda.nccl.version())
        info['torch'] = torch.__version__
        info['hip'] = getattr(torch.version, 'hip', None)
    except Exception as exc:              # noqa: BLE001
        info['version_error'] = str(exc)
    info['env'] = {k: v for k, v in sorted(os.environ.items())
                   if k.startswith(('NCCL_', 'RCCL_', 'HSA_ENABLE_IPC', 'HSA_FORCE', 'HIP_VISIBLE', 'ROCR_VISIBLE'))}
    info['nccl_algo_set'] = 'NCCL_ALGO' in os.environ
    links = {'xgmi': 0, 'pcie': 0}
    try:                                   # KFD topology: io_links/*/properties, type 11 = xGMI, 2 = PCIe
        base = '/sys/class/kfd/kfd/topology/nodes'
        for node in sorted(os.listdir(base)):
            d = os.path.join(base, node, 'io_links')
            if not os.path.isdir(d):
                continue
            for link in os.listdir(d):
                with open(os.path.join(d, link, 'properties')) as fid:
                    props = dict(line.split()[:2] for line in fid if len(line.split()) >= 2)
                t = int(props.get('type', -1))
                if t == 11:
                    links['xgmi'] += 1
                elif t == 2:
                    links['pcie'] += 1
        info['io_links_seen'] = links
    except (OSError, ValueError):
        info['io_links_seen'] = None
    return info


OTHER_LEGS = [('cfg1', False), ('cfg3', False), ('cfg5', False), ('cfg2', True), ('cfg3', True), ('cfg5', True)]


def other_configs(args, server):
    '''The other single-GPU configs of BASELINE.json — configs[0] (cfg1), configs[2] (cfg3), one GPU's share of
    configs[4] (cfg5) — and the cfg2 / cfg3 / cfg5 recipes with the REFERENCE's regularisation defaults switched on
    (training_defaults), each timed in this same command with the headline's bracket (3 warm-up steps, --other-steps
    timed steps, device sync on both sides): their numbers are then in the driver's record, not only in profiles/.'''
    import torch
    out = {'protocol': '3 warm-up + %d timed steps each, sync bracket, same process as the headline' % args.other_steps}
    for w, td in OTHER_LEGS:
        a = argparse.Namespace(**vars(args))
        a.workload, a.training_defaults, a.steps, a.warmup = w, td, args.other_steps, 3
        a.gemm_precision, a.no_gemm_roofline, a.no_alt, a.allreduce = None, True, True, 'flat'
        key = w if not td else 'training_defaults'
        try:
            wl = HipWorkload(a, server)
            for i in range(a.warmup):
                wl.step(i)
            wl.check()
            wl.sync()
            wl.start_timed_region()
            t0 = time.perf_counter()
            for i in range(a.steps):
                wl.step(i)
            wl.sync()
            dt = time.perf_counter() - t0
            wl.end_timed_region()
            wl.check()
            d = wl.describe(dt)
            rk = d['roofline']['recurrent_kernels']
            entry = {'metric': d['metric'], 'workload': d['config']['workload'], 'ms_per_step': round(dt / a.steps * 1e3, 3),
                     'value': round(wl.units_per_step * a.steps / dt, 2), 'unit': 'utterances/sec', 'steps': a.steps, 'warmup': a.warmup,
                     'final_loss': d['final_loss'], 'dtype': d['dtype'], 'recurrent_path': d['config']['recurrent_path'],
                     'decoder_persistent': wl.rank_paths()[1],
                     'roofline_frac_step': d['roofline']['frac'],
                     'recurrent_kernels': {'frac': rk['frac'], 'us_per_sequential_step': rk['us_per_sequential_step'],
                                           'ms_per_step': rk['ms_per_step']},
                     'effective_clock': wl.effective_clock()}
            if d.get('roofline_decoder'):
                entry['roofline_decoder'] = d['roofline_decoder']
            del wl
        except Exception as exc:          # noqa: BLE001 — one leg must not take the headline's line down
            entry = {'error': '%s: %s' % (type(exc).__name__, exc)}
        torch.cuda.empty_cache()
        if td:
            out.setdefault('training_defaults', {
                'note': 'the same recipes with the reference\'s regularisation defaults ON: Listener input_noise 0.6 + dropout '
                        'keep 0.5 (ed_encoders/defaults/listener.cfg), Speller dropout 0.5 + sample_prob 0.1 '
                        '(ed_decoders/defaults/speller.cfg); BASELINE.json\'s configs state none, so the headline has none'})[w] = entry
        else:
            out[w] = entry
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    env_world = int(os.environ.get('WORLD_SIZE', '1'))
    if args.gpus > 1 and env_world == 1:
        # no ranks in the environment: start them ourselves
        sys.exit(self_launch(argv, args.gpus))
    if args.cpu_all_cores:
        from oracle import cpu_baseline as cb
        phys = cb.physical_cores()
        r = cb.time_config('cfg2', 0, 1, threads=phys)
        print(json.dumps({'cpu_all_physical_cores': {'workload': 'cfg2', 'cores': phys, 'logical': os.cpu_count(),
                                                     'seconds_per_step': r['seconds_per_step'], 'value': r['utt_per_s'],
                                                     'unit': 'utterances/sec', 'kind': 'port', 'warmup': 0,
                                                     'steps': r['steps_timed'], 'host': socket.gethostname()}}), flush=True)
        sys.exit(0)
    if args.dry_run:
        sys.exit(dry_run(args))
    server = make_server()
    if server.world_size != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d' % (args.gpus, server.world_size))
    wl = make_workload(args, server)
    out = run(args, server, wl)
    if out is not None:
        print(json.dumps(out), flush=True)
    server.barrier()
    server.shutdown()


def alt_gemm_arith(tr, batches, server, steps, warmup, keys):
    """the same step with another arithmetic of the BLSTM layers' dense products (exact fp32 / bf16x6 / f16x3) and / or of
    their recurrent product: the encoder's cfg keys (gemm_precision, recurrent_precision) are switched for the duration
    (the layers read them at every call), timed with the protocol, warm-up and step count of the headline; NOT the
    headline value"""
    import torch
    conf = tr.model.encoder.conf
    restore = {k: conf.get(k, None) for k in keys}
    conf.update(keys)
    try:
        for i in range(warmup):
            tr.step(batches[i % 2])
        torch.cuda.synchronize()
        server.barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            loss = tr.step(batches[i % 2])
        torch.cuda.synchronize()
        server.barrier()
        dt = time.perf_counter() - t0
    finally:
        for k, v in restore.items():
            if v is None:
                del conf[k]
            else:
                conf[k] = v
    return dt, float(loss.item())


if __name__ == '__main__':
    main()
