"""What Trainer.train() delivers against the bare step bench.py times, with and without the overlapped loop
(prefetch_batches), for cfg2 and cfg3 at full size (32 x 1000 x 40).  One process, one JSON line:

  (a) bare_ms        the step the way bench.py times it: two resident batches, no read-back, a device-synchronised
                     window behind a warm-up;
  (b) sync_ms        Trainer.train() with prefetch_batches = 0;
  (c) overlap_ms     Trainer.train() with prefetch_batches = 2;
  producer_ms        ms per staged batch from the prefetcher alone (the configured workers, no GPU work): together with
                     (a) it bounds what (c) can reach,
each of (b), (c) and the producer on two sources: SyntheticData and a TFRecord data set written to a temporary
directory with the repo's own writers.  (b) and (c) alternate (--rounds of each, the median is reported); a window
covers --steps whole iterations of the loop behind --warmup iterations, between two device synchronisations.  For (c)
the line also says where an iteration's host time goes: enqueueing (upload + unpack + the step's launches), waiting
for a batch (worker starvation) and waiting for the lagged record (the device is the bound: the wanted state).

    python tools/train_loop_bench.py [--steps 50] [--warmup 5] [--rounds 2] [--workers 2] [--only cfg2|cfg3]

Needs a GPU; there is no fallback."""
import argparse
import contextlib
import gc
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nabu_amd import recipes                                                  # noqa: E402
from nabu_amd.neuralnetworks.trainers import readback, trainer_factory        # noqa: E402
from nabu_amd.processing import prefetch                                      # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402
from nabu_amd.processing.tfwriters import tfwriter_factory                    # noqa: E402

B, T, D = 32, 1000, 40
WORKLOADS = {
    'cfg2': dict(recipe='cfg2_listener_ctc', eos=False,
                 data=dict(min_frames=T, min_labels=20, max_labels=60, time_reduction=8, seed=4234)),
    'cfg3': dict(recipe='cfg3_las_vanilla', eos=True,
                 data=dict(min_frames=T, min_labels=20, max_labels=79, eos=True, time_reduction=8, seed=3234)),
}


def write_dataset(root, eos, utterances=8 * B, seed=0):
    """a `run data` directory pair (features + text) of utterances of T frames each, like the synthetic workload's
    (min_frames = T), so that a step on them is the step (a) times; returns the database conf"""
    import configparser
    rng = np.random.default_rng(seed)
    alphabet = ['s%02d' % i for i in range(39)]
    fdir, tdir = os.path.join(root, 'fbank'), os.path.join(root, 'text')
    fw, tw = tfwriter_factory.factory('array')(fdir), tfwriter_factory.factory('string')(tdir)
    flens, tlens = [], []
    for i in range(utterances):
        frames = T
        labels = int(rng.integers(20, 61))                     # fits T / 8 encoder frames with every repeat
        fw.write(rng.standard_normal((frames, D)).astype(np.float32), 'utt%04d' % i)
        tw.write(' '.join(alphabet[j] for j in rng.integers(0, 39, labels)), 'utt%04d' % i)
        flens.append(frames)
        tlens.append(labels)
    for d, lens in ((fdir, flens), (tdir, tlens)):
        with open(os.path.join(d, 'max_length'), 'w') as fid:
            fid.write(str(max(lens)))
        np.save(os.path.join(d, 'sequence_length_histogram.npy'), np.bincount(lens, minlength=max(lens) + 1))
    for path, text in ((os.path.join(fdir, 'dim'), str(D)), (os.path.join(tdir, 'alphabet'), ' '.join(alphabet)),
                       (os.path.join(tdir, 'nonesymbol'), '<none>')):
        with open(path, 'w') as fid:
            fid.write(text)
    conf = configparser.ConfigParser()
    conf.read_dict({'trainfbank': {'type': 'audio_feature', 'dir': fdir},
                    'traintext': {'type': 'string_eos' if eos else 'string', 'dir': tdir}})
    return conf


def make_trainer(name, source, total_steps, prefetch_batches, workers):
    w = WORKLOADS[name]
    mc, tc, ec = recipes.load_recipe(w['recipe'], **{'evaluator.evaluator': 'None', 'trainer.num_epochs': 1,
                                                     'trainer.numbuckets': 1})
    tc.set('trainer', 'prefetch_batches', str(prefetch_batches))
    tc.set('trainer', 'prefetch_workers', str(workers))
    for key, section in (('features', 'trainfbank'), ('targets', 'text'), ('text', 'traintext')):
        tc.set('trainer', key, section)
    if source == 'synthetic':
        data = SyntheticData(B, T, D, batches_per_epoch=total_steps, **w['data'])
    else:
        data = source                                          # the database conf of write_dataset
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=None, task_index=0)
    tr._create_graph()
    tr._graph['num_steps'] = total_steps                       # (the record set is walked over several epochs)
    return tr


def bare_step_ms(name, steps, warmup):
    tr = make_trainer(name, 'synthetic', steps, 0, 1)
    batches = [tr.to_device(tr.data.batch(i)) for i in range(2)]
    for i in range(warmup):
        tr.step(batches[i % 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(batches[i % 2])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    from nabu_amd.neuralnetworks.trainers import loss_functions
    loss_functions.check_status()
    return ms


def train_loop_ms(name, source, steps, warmup, prefetch_batches, workers):
    """ms per iteration of Trainer.train() over `steps` whole iterations, and the host's share of them"""
    tr = make_trainer(name, source, warmup + steps + 1, prefetch_batches, workers)
    marks, spent = {}, {'enqueue': 0.0, 'get_wait': 0.0, 'read_wait': 0.0}
    calls = {'n': 0}
    plain_step, plain_staged = tr.step, tr.to_device_staged
    plain_get, plain_read = prefetch.BatchPrefetcher.get, readback.StepRecord.read

    def timed(key, fn):
        def call(*args, **kwargs):
            t = time.perf_counter()
            try:
                return fn(*args, **kwargs)
            finally:
                if 'start' in marks and 'end' not in marks:
                    spent[key] += time.perf_counter() - t
        return call

    def step(batch):
        if calls['n'] in (warmup, warmup + steps):             # the window: `steps` whole iterations
            torch.cuda.synchronize()
            marks['start' if calls['n'] == warmup else 'end'] = time.perf_counter()
        calls['n'] += 1
        return timed('enqueue', plain_step)(batch)
    tr.step, tr.to_device_staged = step, timed('enqueue', plain_staged)
    prefetch.BatchPrefetcher.get = timed('get_wait', plain_get)
    readback.StepRecord.read = timed('read_wait', plain_read)
    try:
        with contextlib.redirect_stdout(io.StringIO()):        # the loop prints every step
            hist = tr.train()
    finally:
        prefetch.BatchPrefetcher.get, readback.StepRecord.read = plain_get, plain_read
        if hasattr(tr.data, 'close'):
            tr.data.close()
    assert len(hist) == warmup + steps + 1 and all(np.isfinite(h[1]) for h in hist)
    del tr
    gc.collect()
    out = {'ms': (marks['end'] - marks['start']) * 1e3 / steps}
    out.update({k + '_ms': v * 1e3 / steps for k, v in spent.items()})
    return out


def producer_ms(name, source, batches, workers):
    """ms per staged batch of the prefetcher alone (no device work; the staging memory is not pinned here)"""
    tr = make_trainer(name, source, batches + 8, 0, 1)
    pf = prefetch.BatchPrefetcher(tr.data, 0, 1, 2, workers, prefetch.stage)
    try:
        for _ in range(4):
            pf.get()
        t0 = time.perf_counter()
        for _ in range(batches):
            pf.get()
        return (time.perf_counter() - t0) * 1e3 / batches
    finally:
        pf.close()
        if hasattr(tr.data, 'close'):
            tr.data.close()


def measure(name, args, tmp):
    res = {'bare_ms': bare_step_ms(name, args.steps, args.warmup)}
    sources = {'synthetic': 'synthetic', 'tfrecord': write_dataset(os.path.join(tmp, name), WORKLOADS[name]['eos'])}
    for label, source in sources.items():
        runs = {0: [], 2: []}
        for _ in range(args.rounds):                           # (b) and (c) alternate
            for depth in (0, 2):
                runs[depth].append(train_loop_ms(name, source, args.steps, args.warmup, depth, args.workers))
                print('%s %s prefetch_batches = %d: %.3f ms' % (name, label, depth, runs[depth][-1]['ms']),
                      file=sys.stderr, flush=True)
        sync = sorted(runs[0], key=lambda r: r['ms'])[len(runs[0]) // 2]
        over = sorted(runs[2], key=lambda r: r['ms'])[len(runs[2]) // 2]
        prod = producer_ms(name, source, min(args.steps, 32), args.workers)
        bound = max(res['bare_ms'], prod)
        res[label] = {'sync_ms': sync['ms'], 'overlap_ms': over['ms'], 'producer_ms': prod,
                      'sync_over_bare': sync['ms'] / res['bare_ms'], 'overlap_over_bare': over['ms'] / res['bare_ms'],
                      'overlap_over_bound': over['ms'] / bound, 'meets_bar': over['ms'] <= 1.03 * bound,
                      'overlap_host': {k: over[k] for k in ('enqueue_ms', 'get_wait_ms', 'read_wait_ms')},
                      'sync_host': {k: sync[k] for k in ('enqueue_ms',)},
                      'all_sync_ms': [r['ms'] for r in runs[0]], 'all_overlap_ms': [r['ms'] for r in runs[2]]}
    res['bare_ms_after'] = bare_step_ms(name, args.steps, args.warmup)
    return res


def rounded(x):
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    if isinstance(x, list):
        return [rounded(v) for v in x]
    return round(x, 3) if isinstance(x, float) else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50, help='timed iterations per window (at least 50 for a record)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--workers', type=int, default=2)
    ap.add_argument('--only', choices=sorted(WORKLOADS), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('train_loop_bench needs a GPU (the HIP path has no CPU fallback)')
    torch.cuda.set_device(0)
    out = {'bench': 'train_loop_overlap', 'shape': [B, T, D], 'steps': args.steps, 'warmup': args.warmup,
           'rounds': args.rounds, 'prefetch_batches': 2, 'prefetch_workers': args.workers,
           'device': torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(WORKLOADS):
            if args.only in (None, name):
                out[name] = measure(name, args, tmp)
    print(json.dumps(rounded(out)), flush=True)


if __name__ == '__main__':
    main()
