"""CTC test cases and their yardstick (plain NumPy; importable without a GPU).

make_case() builds the inputs of one case, judge() compares a kernel's result with the float64 oracle
(oracle.nabu_oracle.ctc_loss) using the SAME oracle run in float32 as the measure of what float32 log-space
arithmetic can deliver on that case, and CASES is the table both the in-process test (tests/test_hip_ctc.py) and
the child process (tests/ctc_kernel_check.py) iterate over.  tests/test_ctc_cases.py holds all of it to its own
promises on the CPU."""
import collections

import numpy as np

from oracle import nabu_oracle as O

REGIMES = ('random', 'peaky', 'aligned')
LATTICES = ('loose', 'tight')
SIGMA = {'random': 2.0, 'peaky': 12.0, 'aligned': 2.0}
BOOST = 10.0             # 'aligned': added to the logit of the alignment's class at every frame
U = 2.0 ** -24           # unit roundoff of float32
# judge()'s allowance over the float32 oracle's own error.  K = 4: per frame the wave kernel adds one rounding for the
# base-2 scaling and uses 1-ulp exp2 / log2 where NumPy's libm is within 0.5 ulp — about twice the roundings of the
# float32 restatement — and the errors of the alpha and the beta sweep add.  Gradients and frame sums of both kernels
# are held to it: both sides of that comparison are maxima over B*T*C (B*T) entries, a stable statistic.
K = 4.0
# The nll is different: where one long utterance decides the case (every tight lattice: utterance 0 keeps the full
# length, the others have a single path), kernel and float32 oracle each contribute ONE number, the end of a random
# walk of per-frame roundings at an ulp of |alpha| — 2 per frame on the chain of either kernel (max + log(sum),
# + emission), 3 in the oracle (two two-term log-sum-exps, + emission); the wave kernel's lattice is in bits
# (1.4427 ln p), which for |ln p| in (2^k / 1.4427, 2^k) sits one binade higher and rounds 2 ln 2 = 1.39 times as
# coarsely, otherwise 0.69 times.  Equal RMS on both sides, then, and the quotient of two such draws is half-Cauchy:
# it exceeds r with probability (2/pi) atan(1/r) — 15.6 % for r = 4, 4 % for r = 16 — for a PERFECT float32 kernel.
# Seen on the MI355X: (4, 140, 40, 62) random/tight, utterance 0, nll 489.7: the oracle's float32 draw is off by
# 2.0e-5 nats (0.7 ulp), a ninth of ITS RMS (sqrt(3 * 140) * 0.29 * 3.05e-5 = 1.8e-4); the wave kernel by 1.4e-4
# (RMS of its 2 * 140 roundings of 2^-14 bits: 2.0e-4), ctc_kernel by 1.3e-4: quotients 6.9 and 6.6.  And
# (3, 235, 40, 60) aligned/tight, utterance 0, nll 20.68: ctc_kernel 8 ulp, the oracle 1.2 ulp, quotient 6.6 —
# the one case that needs more than 4 once the floor is taken off (4.46).
# So the nll is held to the largest allowance the yardstick admits, 16; its gradient (which contains exp(nll)) to 4.
K_NLL = 16.0


# ---------------------------------------------------------------------------------------------------------------
# which kernel nabu_ctc_loss_grad takes (csrc/ctc.hip: ctc_wave_lds_bytes and the dispatch condition) and from which
# request on its launch raises the LDS attribute (csrc/common.hip: ensure_dynamic_lds, behind launch_lds); held to the
# source text by tests/test_ctc_cases.py::test_lds_formula_is_the_one_in_the_source
WAVE_LDS_FORMULA = ('((size_t)T * C + (size_t)T * Smax + C + 64 + 2 + 3 * 64 + 3 * (size_t)C) * sizeof(float) '
                    '+ (128 + 2) * sizeof(int)')
WAVE_DISPATCH = '!force_wg && Lmax <= 63 && wshm <= 150 * 1024'
WAVE_ATTR = 'if (bytes > 64 * 1024) {'
WAVE_LAUNCH = 'return launch_lds(ctc_wave_kernel, dim3(B), dim3(256), wshm, s, p);'


def wave_lds_bytes(T, C, Lmax):
    Smax = 2 * Lmax + 1
    return (T * C + T * Smax + C + 64 + 2 + 3 * 64 + 3 * C) * 4 + (128 + 2) * 4


def wave_eligible(T, C, Lmax):
    """the default dispatch takes ctc_wave_kernel (otherwise ctc_kernel, as NABU_CTC_WORKGROUP=1 does for every shape)"""
    return Lmax <= 63 and wave_lds_bytes(T, C, Lmax) <= 150 * 1024


def largest_T_within(limit, C, Lmax):
    T = 1
    while wave_lds_bytes(T + 1, C, Lmax) <= limit:
        T += 1
    return T


# ---------------------------------------------------------------------------------------------------------------
class Case(object):
    """inputs of one case: logits float32 [B,T,C], logit_len / label_len int32 [B], labels int32 [B,Lmax];
    need[b] = max(1, label_len + adjacent repeats) is the shortest logit_len with a valid alignment"""

    def __init__(self, logits, logit_len, labels, label_len, need, meta):
        self.logits, self.logit_len, self.labels, self.label_len, self.need = logits, logit_len, labels, label_len, need
        self.meta = meta
        self._oracle = None

    def __iter__(self):
        return iter((self.logits, self.logit_len, self.labels, self.label_len))

    @property
    def shape(self):
        return self.logits.shape + (self.labels.shape[1],)

    def oracle(self):
        """(n64, g64, n32, g32): the oracle on the float32 logits in float64, and the same code run in float32"""
        if self._oracle is None:
            n64, g64 = O.ctc_loss(self.logits.astype(np.float64), self.logit_len, self.labels, self.label_len)
            with np.errstate(over='ignore', under='ignore'):
                n32, g32 = O.ctc_loss(self.logits, self.logit_len, self.labels, self.label_len)
            assert n32.dtype == np.float32 and g32.dtype == np.float32
            self._oracle = (n64, g64, n32.astype(np.float64), g32.astype(np.float64))
        return self._oracle


def needed_frames(labels, label_len):
    need = np.zeros(len(label_len), np.int64)
    for b, L in enumerate(label_len):
        lab = labels[b, :L]
        need[b] = max(1, int(L) + int(np.sum(lab[1:] == lab[:-1])))
    return need


def _alignment(rng, lab, Tb, blank):
    """a uniformly drawn-ish VALID alignment of `lab` over Tb frames: the shortest one (labels, a blank between
    adjacent repeats; one blank for an empty label) with the remaining frames handed out at random to the 2L+1
    slots (blank, label, blank, ..., label, blank)"""
    L = len(lab)
    count = np.zeros(2 * L + 1, np.int64)
    count[1::2] = 1
    for i in range(1, L):
        if lab[i] == lab[i - 1]:
            count[2 * i] = 1
    if L == 0:
        count[0] = 1
    extra = Tb - int(count.sum())
    assert extra >= 0
    if extra:
        count += np.bincount(rng.integers(0, 2 * L + 1, extra), minlength=2 * L + 1)
    ext = np.full(2 * L + 1, blank, np.int64)
    ext[1::2] = lab
    return np.repeat(ext, count)


def make_case(B, T, C, Lmax, regime, lattice, seed):
    """float32 logits, logit_len, labels, label_len (a Case unpacks into these four).

    regime:  'random' N(0, 2) | 'peaky' N(0, 12) | 'aligned' N(0, 2) plus BOOST on the class of a randomly drawn valid
             alignment at every frame (the logits of a model that has learnt its alignment: small nll)
    lattice: 'loose' logit_len in [max(need, T/2), T] | 'tight' logit_len = need (a single valid path)
    Utterance 0 always has the full length T (also in a tight case — it is the one exception there) and an adjacent
    repeat (Lmax >= 2); the last has label_len = Lmax; utterance 1 has label_len = 0 when B >= 3.  Labels, lengths
    and the noise depend on the seed alone, so the regimes and lattices of one seed are comparable."""
    assert regime in REGIMES and lattice in LATTICES
    rng = np.random.default_rng(seed)
    label_len = rng.integers(0, Lmax + 1, B)
    labels = rng.integers(0, C - 1, (B, Lmax))
    u = rng.random(B)
    noise = rng.standard_normal((B, T, C))
    if Lmax >= 2:
        label_len[0] = max(label_len[0], 2)
        labels[0, 1] = labels[0, 0]
    if B >= 3:
        label_len[1] = 0
    label_len[-1] = Lmax
    need = needed_frames(labels, label_len)
    assert np.all(need <= T), (need, T)
    if lattice == 'tight':
        logit_len = need.copy()
    else:
        lo = np.maximum(need, T // 2)
        logit_len = lo + np.floor(u * (T - lo + 1)).astype(np.int64)
    logit_len[0] = T
    logits = SIGMA[regime] * noise
    if regime == 'aligned':
        arng = np.random.default_rng([seed, 1])
        for b in range(B):
            path = _alignment(arng, labels[b, :label_len[b]], int(logit_len[b]), C - 1)
            logits[b, np.arange(len(path)), path] += BOOST
    meta = dict(B=B, T=T, C=C, Lmax=Lmax, regime=regime, lattice=lattice, seed=seed)
    return Case(np.ascontiguousarray(logits, np.float32), logit_len.astype(np.int32), labels.astype(np.int32),
                label_len.astype(np.int32), need, meta)


# ---------------------------------------------------------------------------------------------------------------
Verdict = collections.namedtuple('Verdict', 'ok report e_ref e_ker s_ref s_ker n_ref n_ker')


def _ratio(ker, ref):
    return ker / ref if ref > 0 else (0.0 if ker == 0 else float('inf'))


def judge(nll, dlogits, case, grad_scale=1.0, k=K, k_nll=K_NLL):
    """Compare a result (nll [B], dlogits [B,T,C] = grad_scale * dnll/dlogits) with the float64 oracle, allowing k
    times what the float32 oracle itself loses on this case:
      gradient    e_ker = max|dlogits/grad_scale - g64|         <= k * max|g32 - g64| + 8 * 2^-24
      frame sums  s_ker = max_{b,t<len} |sum_c dlogits|/scale   <= k * max |sum_c g32| + 8 * 2^-24   (exactly 0 in g64)
      nll         n_ker = max_b |nll - n64| / |n64|             <= k_nll * max_b |n32 - n64| / |n64| + 4 * 2^-24
    Returns a Verdict; .report names the worst entry of every quantity that is out of bounds."""
    n64, g64, n32, g32 = case.oracle()
    nll = np.asarray(nll, np.float64)
    g = np.asarray(dlogits, np.float64) / grad_scale
    assert nll.shape == n64.shape and g.shape == g64.shape, (nll.shape, g.shape)
    valid = np.arange(g.shape[1])[None, :] < np.asarray(case.logit_len)[:, None]
    msgs = []

    e_ref = float(np.abs(g32 - g64).max())
    d = np.abs(g - g64)
    e_ker = float(d.max()) if np.all(np.isfinite(d)) else float('inf')
    if not e_ker <= k * e_ref + 8 * U:
        b, t, c = np.unravel_index(np.argmax(np.where(np.isfinite(d), d, np.inf)), d.shape)
        msgs.append('gradient: e_ker %.3e > %g * e_ref %.3e + 8u at [b %d, t %d, c %d]: %.9g, oracle %.9g'
                    % (e_ker, k, e_ref, b, t, c, g[b, t, c], g64[b, t, c]))

    s_ref = float(np.abs(np.where(valid, g32.sum(2), 0)).max())
    s = np.abs(np.where(valid, g.sum(2), 0))
    s_ker = float(s.max()) if np.all(np.isfinite(s)) else float('inf')
    if not s_ker <= k * s_ref + 8 * U:
        b, t = np.unravel_index(np.argmax(np.where(np.isfinite(s), s, np.inf)), s.shape)
        msgs.append('frame sums: s_ker %.3e > %g * s_ref %.3e + 8u at [b %d, t %d]' % (s_ker, k, s_ref, b, t))

    n_ref = float((np.abs(n32 - n64) / np.abs(n64)).max())
    r = np.abs(nll - n64) / np.abs(n64)
    n_ker = float(r.max()) if np.all(np.isfinite(r)) else float('inf')
    if not n_ker <= k_nll * n_ref + 4 * U:
        b = int(np.argmax(np.where(np.isfinite(r), r, np.inf)))
        msgs.append('nll: n_ker %.3e > %g * n_ref %.3e + 4u at [b %d]: %.9g, oracle %.9g'
                    % (n_ker, k_nll, n_ref, b, nll[b], n64[b]))
    return Verdict(not msgs, '; '.join(msgs), e_ref, e_ker, s_ref, s_ker, n_ref, n_ker)


def ratios(v):
    """(gradient, frame-sum, nll) error of the judged result as multiples of the float32 oracle's"""
    return _ratio(v.e_ker, v.e_ref), _ratio(v.s_ker, v.s_ref), _ratio(v.n_ker, v.n_ref)


def needed(v):
    """the smallest allowances with which judge() accepts the result: (error - floor) / reference error, >= 0"""
    return (_ratio(max(v.e_ker - 8 * U, 0.0), v.e_ref), _ratio(max(v.s_ker - 8 * U, 0.0), v.s_ref),
            _ratio(max(v.n_ker - 4 * U, 0.0), v.n_ref))


# ---------------------------------------------------------------------------------------------------------------
# The case table.  (group, why, shapes (B, T, C, Lmax), regimes, lattices); every shape with wave_eligible() runs
# twice on the GPU — default dispatch (ctc_wave_kernel) in the pytest process, NABU_CTC_WORKGROUP=1 (ctc_kernel) in a
# child process per group; a shape the wave kernel cannot take runs once, on ctc_kernel, in the pytest process.
LDS_C, LDS_LMAX = 40, 60
T64 = largest_T_within(64 * 1024, LDS_C, LDS_LMAX)      # 98: the last T below the raised-LDS-attribute launch
T150 = largest_T_within(150 * 1024, LDS_C, LDS_LMAX)    # 235: the last T the wave kernel takes

ALL = (REGIMES, LATTICES)
TABLE = [
    # lane 63 holds the last blank state at Lmax = 63; Lmax = 64 is the first shape of the workgroup kernel (runs once)
    ('lanes', 'lane 63 / last blank state; the Lmax <= 63 switch',
     [(4, 140, 40, 62), (4, 140, 40, 63), (4, 140, 40, 64)]) + ALL,
    # S = 255 / 257 states over 256 threads; Lmax > 63: workgroup kernel only (run once)
    ('states', '256-thread state stride of the workgroup kernel', [(3, 300, 40, 127), (3, 300, 40, 128)]) + ALL,
    ('classes', 'class strides 64 (wave kernel), 192 and 256 (workgroup kernel)',
     [(4, 40, 64, 10), (4, 40, 65, 10), (4, 40, 193, 10), (4, 30, 257, 8), (3, 24, 300, 8)]) + ALL,
    ('small', 'smallest legal problems; Lmax = 0 is an empty label tensor', [(1, 1, 2, 0), (2, 1, 2, 1), (3, 2, 3, 1)]) + ALL,
    # T150 + 1 does not fit the wave kernel: workgroup kernel, runs once
    ('lds', 'wave-kernel LDS just under / over 64 KiB (attribute raised) and 150 KiB (workgroup kernel instead)',
     [(3, T64, LDS_C, LDS_LMAX), (3, T64 + 1, LDS_C, LDS_LMAX), (3, T150, LDS_C, LDS_LMAX),
      (3, T150 + 1, LDS_C, LDS_LMAX)]) + ALL,
    ('odd', 'odd C*T: utterance 1 is not 16-byte aligned (scalar staging) next to aligned ones', [(3, 33, 41, 12)]) + ALL,
    ('full', 'cfg2 at full size', [(32, 125, 40, 60)]) + ALL,
    # T = 1000 does not fit the wave kernel's LDS: workgroup kernel, runs once
    ('full', 'cfg1 at full size', [(8, 1000, 40, 60)], ('random', 'aligned'), ('loose',)),
]
SCALE_SHAPE = (4, 40, 65, 10)          # grad_scale != 1: 1/B and 0.37 ('random', 'loose')


def seed_of(B, T, C, Lmax):
    return 100000 * B + 100 * T + 7 * C + 13 * Lmax


def _table():
    cases = []
    for group, why, shapes, regimes, lattices in TABLE:
        for shape in shapes:
            for regime in regimes:
                for lattice in lattices:
                    cases.append(dict(id='%dx%dx%dx%d-%s-%s' % (shape + (regime, lattice)), group=group, shape=shape,
                                      regime=regime, lattice=lattice, grad_scale=1.0))
    for name, scale in (('1/B', 1.0 / SCALE_SHAPE[0]), ('0.37', 0.37)):
        cases.append(dict(id='%dx%dx%dx%d-random-loose-scale%s' % (SCALE_SHAPE + (name.replace('/', 'over'),)),
                          group='scale', shape=SCALE_SHAPE, regime='random', lattice='loose', grad_scale=scale))
    return cases


CASES = _table()
GROUPS = sorted(set(c['group'] for c in CASES if wave_eligible(*c['shape'][1:])))    # groups with a forced-kernel run


def build(entry):
    B, T, C, Lmax = entry['shape']
    return make_case(B, T, C, Lmax, entry['regime'], entry['lattice'], seed_of(B, T, C, Lmax))
