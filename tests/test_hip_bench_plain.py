"""GPU: a plain bench.py run (no --full) of the headline workload (cfg2): the line carries the headline and what the
timed steps themselves recorded, none of the legs that take runs of their own, and the run spends little time outside
its warm-up and timed steps."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                         # noqa: E402


def test_plain_run_is_the_headline_only():
    steps, warmup = 4, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                        '--warmup', str(warmup)], capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert line['metric'] == bench.METRICS['cfg2'] and line['unit'] == 'utterances/sec' and line['higher_is_better'] is True
    assert line['dtype'] and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['ms_per_step_repeats'] == [line['ms_per_step']] and line['roofline_gemm'] is None
    assert not {'cpu_baseline', 'other_configs', 'alt_bf16x6', 'alt_f16x3', 'f32_products', 'fp32_end_to_end'} & set(line)
    assert line['roofline']['recurrent_kernels']['launches_timed'] > 0
    # start-up, the first step's code loading and teardown included: at most 30 s besides the steps themselves
    assert wall - (steps + warmup) * line['ms_per_step'] * 1e-3 < 30.0, wall
