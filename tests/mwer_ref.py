"""Host restatement of the MWER kernels (nabu_amd/csrc/mwer.hip): prepare, tile and loss / gradient in numpy, float64 by
default; `dtype=np.float32` runs the same formulas in float32 (the figure the GPU test's bars are derived from).
Rows are stacked slot-major: row n * B + b is hypothesis n of utterance b, slot N is the reference."""
import numpy as np

REAL_SCORE = -1e30          # a hypothesis with a score above this one exists; the search fills spare slots with -FLT_MAX
FLT_MAX = float(np.finfo(np.float32).max)


def levenshtein(a, b):
    """plain edit distance of two label sequences"""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def prepare(sequences, lengths, scores, targets, target_len, C, ldt=None):
    """beams -> (stk_targets [(N+1)B, ldt], stk_len [(N+1)B], hyp_len [NB], valid [NB]), all int32.  A slot is valid when
    its score is a real one and no lower slot of the utterance with a real score holds the same labels [:length]."""
    sequences = np.asarray(sequences).reshape(np.shape(sequences)[0], np.shape(sequences)[1], -1)
    B, N, S = sequences.shape
    ldr = np.shape(targets)[1]
    ldt = max(S + 1, ldr) if ldt is None else ldt
    assert ldt > S
    stk = np.zeros(((N + 1) * B, ldt), np.int32)
    stk_len = np.zeros((N + 1) * B, np.int32)
    hyp_len = np.zeros(N * B, np.int32)
    valid = np.zeros(N * B, np.int32)
    for b in range(B):
        lens = [min(max(int(lengths[b][n]), 0), S) for n in range(N)]
        real = [bool(scores[b][n] > REAL_SCORE) for n in range(N)]
        for n in range(N):
            hyp = list(sequences[b, n, :lens[n]])
            ok = real[n] and not any(real[m] and list(sequences[b, m, :lens[m]]) == hyp for m in range(n))
            if not ok:
                hyp = []
            row = n * B + b
            stk[row, :len(hyp)] = hyp
            stk[row, len(hyp)] = C - 1
            stk_len[row], hyp_len[row], valid[row] = len(hyp) + 1, len(hyp), int(ok)
        tl = min(max(int(target_len[b]), 0), ldr, ldt)
        stk[N * B + b, :tl] = np.asarray(targets)[b, :tl]
        stk_len[N * B + b] = tl
    return stk, stk_len, hyp_len, valid


def errors(stk_targets, hyp_len, targets, target_len):
    """edit distance of every hypothesis row to its utterance's reference without the end label -> [NB] int32"""
    B = len(target_len)
    return np.array([levenshtein(stk_targets[r, :hyp_len[r]], np.asarray(targets)[r % B, :max(int(target_len[r % B]) - 1, 0)])
                     for r in range(len(hyp_len))], np.int32)


def tile(x, R):
    return np.concatenate([np.asarray(x)] * R, axis=0)


def tile_bwd(dy, R, dtype=np.float64):
    dy = np.asarray(dy, dtype)
    return dy.reshape((R, dy.shape[0] // R) + dy.shape[1:]).sum(axis=0)


def loss_grad(logits, stk_targets, stk_len, errs, valid, ce_weight, grad_scale, dtype=np.float64, with_grad=True):
    """-> (loss [B], risk [B], nll_ref [B], dlogits [(N+1)B, L, C] or None) in `dtype`"""
    x = np.asarray(logits, dtype)
    rows, L, C = x.shape
    NB = len(valid)
    B = rows - NB
    N = NB // B
    ce_weight, grad_scale = dtype(ce_weight), dtype(grad_scale)
    length = np.clip(np.asarray(stk_len), 0, L)
    mask = np.arange(L)[None, :] < length[:, None]                              # [rows, L]
    m = x.max(axis=2, keepdims=True)
    lz = m[..., 0] + np.log(np.exp(x - m).sum(axis=2, dtype=dtype))             # [rows, L]
    y = np.clip(np.asarray(stk_targets)[:, :L], 0, C - 1)
    xy = np.take_along_axis(x, y[:, :, None], axis=2)[..., 0]
    nll = np.where(mask, lz - xy, dtype(0)).sum(axis=1, dtype=dtype)            # [rows]
    nll_h, nll_ref = nll[:NB].reshape(N, B), nll[NB:]
    v = np.asarray(valid).reshape(N, B) != 0
    e = np.asarray(errs).reshape(N, B)
    a = np.where(v, -nll_h, dtype(-np.inf))
    with np.errstate(invalid='ignore', divide='ignore'):
        w = np.where(v, np.exp(a - a.max(axis=0, keepdims=True)), dtype(0)).astype(dtype)
        den = w.sum(axis=0, dtype=dtype)
        p = np.where(v, w / den, dtype(0)).astype(dtype)                        # [N, B]; no valid slot: all zero
    diff = (e[:, None, :] - e[None, :, :]).astype(dtype)                        # [n, m, B] = e_n - e_m, exact
    centred = (p[None, :, :] * diff).sum(axis=1, dtype=dtype)                   # sum_m p_m (e_n - e_m)
    risk = (p * e.astype(dtype)).sum(axis=0, dtype=dtype)
    loss = risk + ce_weight * nll_ref if ce_weight != 0 else risk.copy()
    if not with_grad:
        return loss, risk, nll_ref, None
    coef = np.concatenate([(-grad_scale * (p * centred)).reshape(NB), np.full(B, ce_weight * grad_scale, dtype)])
    soft = np.exp(x - lz[:, :, None])
    onehot = (np.arange(C)[None, None, :] == y[:, :, None]).astype(dtype)
    d = coef[:, None, None] * (soft - onehot)
    d = np.where(mask[:, :, None] & (coef != 0)[:, None, None], d, dtype(0)).astype(dtype)
    return loss, risk, nll_ref, d


# ---- the cases of the loss kernel's test (tests/test_hip_mwer.py); B = 5 throughout
LOSS_B = 5
LOSS_NS, LOSS_LS, LOSS_CS = (1, 2, 4, 16), (1, 19, 300), (2, 41, 1023)
PATTERNS = ('all', 'one', 'slot0')
LOSS_CE_WEIGHT = 0.5


def loss_cases():
    """every (N, L, C) of the three lists, the validity pattern rotating so that every pattern meets every N, L and C;
    and one shape past the LDS route of the kernel ((N + 1) * L > 6144 frames per utterance)"""
    out, k = [], 0
    for N in LOSS_NS:
        for L in LOSS_LS:
            for C in LOSS_CS:
                out.append((N, L, C, PATTERNS[(k + k // 3 + k // 9) % 3]))
                k += 1
    out.append((16, 500, 2, 'all'))
    return out


def case_id(case):
    return 'N%d-L%d-C%d-%s' % case


def loss_inputs(case):
    """seeded inputs of one case: logits float32, stk_targets, stk_len (1 and L among them), errors, valid"""
    N, L, C, pattern = case
    B = LOSS_B
    rng = np.random.RandomState(1000 * N + 10 * L + C + len(pattern))
    rows = (N + 1) * B
    logits = (rng.standard_normal((rows, L, C)) * 2.0).astype(np.float32)
    stk_targets = rng.randint(0, C, size=(rows, L + 2)).astype(np.int32)
    stk_len = rng.randint(1, L + 1, size=rows).astype(np.int32)
    stk_len[0], stk_len[1] = 1, L
    errs = rng.randint(0, 7, size=N * B).astype(np.int32)
    valid = np.zeros((N, B), np.int32)
    if pattern == 'all':
        valid[:] = 1
    elif pattern == 'one':
        valid[rng.randint(0, N, size=B), np.arange(B)] = 1
    else:
        valid[0] = 1
    return logits, stk_targets, stk_len, errs, valid.reshape(-1)


def rel_err(got, want):
    """norm-wise relative error"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.linalg.norm(want.ravel())
    return float(np.linalg.norm((got - want).ravel()) / den) if den else float(np.linalg.norm(got.ravel()))
