"""Timing of the audio front end (nabu_amd/csrc/features.hip): frames per second of the device path on a seeded
synthetic batch (--utts utterances of 3-10 s at 16 kHz, the shipped fbank configuration: 123 columns), against
the float64 host restatement of the tests (tests/feat_ref.py, numpy, one core) on the same batch.

Prints one JSON line: `device_call` counts everything compute_batch does (host plan, copies in, the two launches,
copy out), `device_kernels` the two launches alone (device events).  For information; nothing gates on it.

    python tools/feature_bench.py [--utts 256] [--reps 5] [--host-utts 16]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nabu_amd import _hip                                                                      # noqa: E402
from nabu_amd.processing.processors.feature_computers import feature_computer_factory          # noqa: E402
from tests import feat_ref                                                                      # noqa: E402

RATE = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-utts', type=int, default=16, help='utterances the host restatement is timed on')
    args = ap.parse_args()
    from configparser import ConfigParser
    cfg = ConfigParser()
    cfg.read_dict({'feature': {'feature': 'fbank'}})
    comp = feature_computer_factory.factory('fbank')(cfg)
    rng = np.random.RandomState(0)
    sigs = [feat_ref.speech_like(float(rng.uniform(3.0, 10.0)), RATE, 1000 + i) for i in range(args.utts)]
    feats = comp.compute_batch(sigs, RATE, mvn=True)                 # warm-up (tables, allocator)
    frames = int(sum(f.shape[0] for f in feats))
    calls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        comp.compute_batch(sigs, RATE, mvn=True)
        calls.append(time.perf_counter() - t0)
    # the launches alone
    lib, d, n = _hip.lib(), comp.desc(RATE, True), len(sigs)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int32)
    frame_off, kept = np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
    _hip.check(lib.nabu_feat_plan_host(ctypes.byref(d), n, offsets.ctypes.data, frame_off.ctypes.data,
                                       kept.ctypes.data), 'plan')
    nbytes = lib.nabu_feat_ws_bytes(ctypes.byref(d))
    host = np.zeros(nbytes, np.uint8)
    _hip.check(lib.nabu_feat_tables_host(ctypes.byref(d), host.ctypes.data, nbytes), 'tables')
    dev = [torch.from_numpy(a).cuda() for a in (np.concatenate(sigs), offsets, kept, frame_off, host)]
    out = torch.empty((frames, comp.get_dim()), device='cuda')
    kernels = []
    for _ in range(args.reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _hip.check(lib.nabu_feat_compute(ctypes.byref(d), n, int(np.diff(frame_off).max()), *[_hip.ptr(t) for t in dev[:4]],
                                         _hip.ptr(out), _hip.ptr(dev[4]), nbytes, _hip.stream()), 'compute')
        b.record()
        b.synchronize()
        kernels.append(a.elapsed_time(b) * 1e-3)
    kernels = kernels[2:]
    t0 = time.perf_counter()
    ref = [feat_ref.features(s, RATE) for s in sigs[:args.host_utts]]
    host_s = time.perf_counter() - t0
    host_frames = int(sum(r.shape[0] for r in ref))
    err = max(float(np.abs(f - r).max()) for f, r in zip(feats, ref))
    print(json.dumps({
        'workload': 'fbank 40+energy ddelta mvn, 16 kHz', 'utterances': n, 'frames': frames,
        'audio_seconds': round(float(offsets[-1]) / RATE, 1),
        'device_call_ms': round(1e3 * float(np.median(calls)), 3),
        'device_call_frames_per_s': round(frames / float(np.median(calls))),
        'device_kernels_ms': round(1e3 * float(np.median(kernels)), 3),
        'device_kernels_frames_per_s': round(frames / float(np.median(kernels))),
        'host_float64_utterances': args.host_utts, 'host_float64_frames_per_s': round(host_frames / host_s),
        'max_abs_err_vs_host': err}))


if __name__ == '__main__':
    main()
