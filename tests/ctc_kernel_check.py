"""Body of tests/test_hip_ctc.py: nabu_ctc_loss_grad on the cases of tests/ctc_cases.py — the exact (tolerance-free)
properties of every case and judge() against the float64 / float32 oracle.

check_case() is called in the pytest process (default dispatch), and this file is run as a child process with
NABU_CTC_WORKGROUP=1 (read once per process by csrc/ctc.hip) so that the workgroup kernel meets the shapes the
wave kernel normally takes.  As a program it prints one line per case,
  CASE <id> <kernel> e_ref e_ker s_ref s_ker n_ref n_ker | error ratios gradient frame-sum nll | needed allowances
every failure, and 'CTC OK' at the end if there was none.
usage: python tests/ctc_kernel_check.py GROUP|all [--forced]     (--forced: only shapes the wave kernel would take)"""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import ctc_cases as cc  # noqa: E402


def forced_workgroup():
    return os.environ.get('NABU_CTC_WORKGROUP', '0') not in ('', '0')


def _dev(a, dtype):
    return torch.as_tensor(np.array(a, order='C', copy=True)).to(dtype).cuda()


def run(logits, logit_len, labels, label_len, scale):
    """one call of the kernel on host arrays -> (nll float32 [B], dlogits float32 [B,T,C], status)"""
    from nabu_amd import ops
    nll, dl, status = ops.ctc_loss_grad(_dev(logits, torch.float32), _dev(logit_len, torch.int32), _dev(labels, torch.int32),
                                        _dev(label_len, torch.int32), float(scale))
    return nll.cpu().numpy(), dl.cpu().numpy(), int(status.item())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def exact_failures(case, scale, base, run=run):
    """the properties that hold without a tolerance; `base` = run(*case, scale).  Returns a list of failures."""
    logits, tl, labels, ll = case
    B, T, C = logits.shape
    Lmax = labels.shape[1]
    nll0, dl0, st0 = base
    bad = []

    def expect(cond, what):
        if not cond:
            bad.append(what)

    expect(st0 == 0, 'status %d on a valid batch' % st0)
    expect(nll0.dtype == np.float32 and dl0.dtype == np.float32, 'outputs are not float32')
    expect(bool(np.all(np.isfinite(nll0)) and np.all(np.isfinite(dl0))), 'non-finite output')
    for b in range(B):
        expect(bool(np.all(dl0[b, tl[b]:] == 0)), 'utterance %d: gradient past its length' % b)

    # two calls: same bits
    nll1, dl1, st1 = run(logits, tl, labels, ll, scale)
    expect(st1 == 0 and same_bits(nll1, nll0) and same_bits(dl1, dl0), 'second call differs from the first')

    # batch independence: the reversed batch gives the reversed result
    nllr, dlr, str_ = run(logits[::-1], tl[::-1], labels[::-1], ll[::-1], scale)
    expect(str_ == 0 and same_bits(nllr[::-1], nll0) and same_bits(dlr[::-1], dl0),
           'reversing the batch changes an utterance: %s' % np.flatnonzero(
               [not (same_bits(nllr[::-1][b:b + 1], nll0[b:b + 1]) and same_bits(dlr[::-1][b], dl0[b])) for b in range(B)]))

    # clamping: logit_len > T, label_len > Lmax, label_len < 0
    tl2, ll2 = tl.copy(), ll.copy()
    tl2[0] = T + 5                    # utterance 0 has logit_len = T
    ll2[-1] = Lmax + 3                # the last has label_len = Lmax
    if B >= 3:
        ll2[1] = -2                   # utterance 1 has label_len = 0
    nllc, dlc, stc = run(logits, tl2, labels, ll2, scale)
    expect(stc == 0 and same_bits(nllc, nll0) and same_bits(dlc, dl0), 'lengths beyond T / Lmax (below 0) are not clamped')
    if B < 3:
        ll3, ll4 = ll.copy(), ll.copy()
        ll3[0], ll4[0] = 0, -2
        r3, r4 = run(logits, tl, labels, ll3, scale), run(logits, tl, labels, ll4, scale)
        expect(r3[2] == 0 and r4[2] == 0 and same_bits(r3[0], r4[0]) and same_bits(r3[1], r4[1]),
               'a negative label_len is not label_len = 0')

    # infeasible / invalid utterances next to valid ones: (a) need > logit_len, (b) label = C-1, (c) label < 0,
    # (d) logit_len = 0 — two per batch, on utterance 0 and on the last
    last = B - 1
    for kinds in ((('a', 0), ('b', last)), (('d', 0), ('c', last))):
        tlb, labb = tl.copy(), labels.copy()
        hit = set()
        for kind, u in kinds:
            if kind in 'bc' and ll[u] < 1:
                continue              # no label to spoil (Lmax = 0)
            if kind == 'a':
                tlb[u] = case.need[u] - 1
            elif kind == 'b':
                labb[u, ll[u] - 1] = C - 1
            elif kind == 'c':
                labb[u, 0] = -1
            else:
                tlb[u] = 0
            hit.add(u)
        if not hit:
            continue
        nllb, dlb, stb = run(logits, tlb, labb, ll, scale)
        name = '+'.join('%s@%d' % k for k in kinds)
        expect(stb - 1 in hit, '%s: status %d names none of %s' % (name, stb, sorted(hit)))
        for u in range(B):
            if u in hit:
                expect(bool(np.isposinf(nllb[u])), '%s: nll[%d] = %r, not +inf' % (name, u, nllb[u]))
                expect(bool(np.all(dlb[u] == 0)), '%s: dlogits[%d] is not all zero' % (name, u))
            else:
                expect(same_bits(nllb[u:u + 1], nll0[u:u + 1]) and same_bits(dlb[u], dl0[u]),
                       '%s: valid utterance %d changed' % (name, u))
    return bad


def check_case(entry):
    """-> (report line, list of failures) for one entry of cc.CASES on the kernel this process dispatches to"""
    case = cc.build(entry)
    scale = entry['grad_scale']
    B, T, C, Lmax = entry['shape']
    kernel = 'wave' if cc.wave_eligible(T, C, Lmax) and not forced_workgroup() else 'workgroup'
    base = run(case.logits, case.logit_len, case.labels, case.label_len, scale)
    bad = exact_failures(case, scale, base)
    v = cc.judge(base[0], base[1], case, scale)
    if not v.ok:
        bad.append(v.report)
    line = 'CASE %s %s e %.3e %.3e s %.3e %.3e n %.3e %.3e | %.2f %.2f %.2f | %.2f %.2f %.2f' % (
        (entry['id'], kernel, v.e_ref, v.e_ker, v.s_ref, v.s_ker, v.n_ref, v.n_ker) + cc.ratios(v) + cc.needed(v))
    return line, bad


def main(argv):
    group, forced = argv[0], '--forced' in argv[1:]
    assert forced == forced_workgroup(), 'NABU_CTC_WORKGROUP and --forced must go together'
    todo = [e for e in cc.CASES if group in ('all', e['group']) and (not forced or cc.wave_eligible(*e['shape'][1:]))]
    assert todo, group
    failures = 0
    for e in todo:
        line, bad = check_case(e)
        print(line, flush=True)
        for b in bad:
            print('FAIL %s: %s' % (e['id'], b), flush=True)
        failures += len(bad)
    if failures:
        print('%d failures in %d cases' % (failures, len(todo)))
        return 1
    print('CTC OK %d cases' % len(todo))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
