"""Body of tests/test_hip_launch_lds.py: the process-wide table of dynamic-LDS grants (csrc/common.hip,
ensure_dynamic_lds) under nabu_ctc_loss_grad's wave kernel, in a process of its own so that the table starts empty.

Per device, in this order, shapes (B, T, C, Lmax):
  1. (3, 99, 40, 60)   main thread    just over 64 KiB: the first grant
  2. (3, 235, 40, 60)  main thread    about 150 KiB: the grant must grow
  3. (3, 99, 40, 60)   a fresh thread must not lower the grant (a launch with more LDS than the attribute allows fails)
  4. (3, 235, 40, 60)  main thread    again
Every call must return status 0 and pass judge() against the float64 oracle (tests/ctc_cases.py).  Device 1 follows in
the same process when the machine has one.  Prints one 'STEP <device> <step> ...' line per call, 'DEVICE 1 SKIPPED: why'
where there is no second device, and 'LDS OK' at the end if nothing failed.
usage: python tests/launch_lds_check.py"""
import os
import sys
import threading

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import torch  # noqa: E402

from tests import ctc_cases as cc  # noqa: E402
from tests import ctc_kernel_check as kc  # noqa: E402

SMALL, LARGE = (3, cc.T64 + 1, cc.LDS_C, cc.LDS_LMAX), (3, cc.T150, cc.LDS_C, cc.LDS_LMAX)
STEPS = ((SMALL, False), (LARGE, False), (SMALL, True), (LARGE, False))     # (shape, from a fresh thread)


def one_call(dev, case, out):
    try:
        torch.cuda.set_device(dev)          # the current device is a per-thread setting
        out.append(kc.run(case.logits, case.logit_len, case.labels, case.label_len, 1.0))
    except Exception as e:                  # an error return of the launch arrives here
        out.append(e)


def main():
    assert not kc.forced_workgroup(), 'NABU_CTC_WORKGROUP is set: the wave kernel would not run'
    assert cc.wave_lds_bytes(*SMALL[1:]) > 64 * 1024 and cc.wave_eligible(*LARGE[1:])
    cases = {s: cc.make_case(*s, regime='random', lattice='loose', seed=cc.seed_of(*s)) for s in (SMALL, LARGE)}
    failures = 0
    ndev = torch.cuda.device_count()
    for dev in (0, 1):
        if dev >= ndev:
            print('DEVICE 1 SKIPPED: the machine has %d device(s)' % ndev, flush=True)
            break
        for i, (shape, threaded) in enumerate(STEPS):
            out = []
            if threaded:
                t = threading.Thread(target=one_call, args=(dev, cases[shape], out))
                t.start()
                t.join()
            else:
                one_call(dev, cases[shape], out)
            if isinstance(out[0], Exception):
                verdict = 'FAIL %s: %s' % (type(out[0]).__name__, out[0])
            else:
                nll, dl, status = out[0]
                v = cc.judge(nll, dl, cases[shape])
                verdict = 'OK' if status == 0 and v.ok else 'FAIL status %d %s' % (status, v.report)
            failures += verdict != 'OK'
            print('STEP %d %d %s %d B %s %s' % (dev, i + 1, 'x'.join(map(str, shape)), cc.wave_lds_bytes(*shape[1:]),
                                                'thread' if threaded else 'main', verdict), flush=True)
    if failures:
        print('%d failures' % failures)
        return 1
    print('LDS OK')
    return 0


if __name__ == '__main__':
    sys.exit(main())
