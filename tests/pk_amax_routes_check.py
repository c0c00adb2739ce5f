"""Cases and child-process body of tests/test_hip_pk_amax_routes.py: the exported nabu_pk_amax on both of its kernels.

The library routes by shape (csrc/gemm_pk.hip, pk_amax_owned): pk_amax_kernel (atomicMax) where its workgroups would
meet at most twice per destination word on average, pk_amax_owner_kernel (one owner per word, no atomics) above
that (columns only from 256 columns on) — of the shapes below: rows only from C = 260, columns and both at C >= 260
with enough rows.
NABU_PK_AMAX_ATOMIC=1 (read once per process) sends every shape to the atomic kernel: the child process.

A case: R x C source with leading dimension ld, which arrays are asked for, and how they are pre-filled.  The source
holds normal draws, +-0, denormals, +-Inf and one NaN, an all-zero row (R > 1) and an all-zero column (C > 1); the
columns [C, ld) of every row hold NaN, so a read beyond C shows.  The destinations lie inside a larger buffer:
GUARD words in front, the array padded past R (C) by PAD words, GUARD words behind, all of which must keep their
pattern.
As a program: python tests/pk_amax_routes_check.py OUT.npz — every case on the kernel this process routes to."""
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(here) not in sys.path:
    sys.path.insert(0, os.path.dirname(here))
import numpy as np  # noqa: E402

GUARD, PAD = 32, 8
SENTINEL = 0x5A5A5A5A
ROWS = (1, 255, 256, 257, 513)
COLS = (4, 60, 64, 68, 260, 262, 2048)          # 262: no multiple of 4, the scalar tail of a row's last 16-byte piece
MODES = ('rows', 'cols', 'both')
PREFILLS = ('zero', 'pattern')


def cases():
    out = []
    for R in ROWS:
        for C in COLS:
            for ld in ((C + 3) // 4 * 4, (C + 3) // 4 * 4 + 8):
                for mode in MODES:
                    for pre in PREFILLS:
                        out.append((R, C, ld, mode, pre))
    return out


def owned(R, C, mode):
    """pk_amax_owned of csrc/gemm_pk.hip for one source: the shape takes pk_amax_owner_kernel"""
    rows, cols = mode != 'cols', mode != 'rows'
    if cols and (R > 8192 or C < 256):
        return False
    atomics = (R * ((C + 63) // 64) if rows else 0) + (C * ((R + 255) // 256) if cols else 0)
    words = (R if rows else 0) + (C if cols else 0)
    return atomics > 2 * words


def case_id(c):
    return '%dx%d-ld%d-%s-%s' % c


def source(R, C, ld):
    """float32 [R, ld]; the same for every mode and prefill of a shape"""
    rng = np.random.default_rng(7919 * R + 31 * C + ld)
    x = rng.standard_normal((R, ld)).astype(np.float32)
    x *= np.float32(2.0) ** rng.integers(-6, 7, (1, ld)).astype(np.float32)         # columns of different magnitudes
    n = R * C
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, np.inf, -np.inf], np.float32)
    pos = rng.choice(n, min(n, 3 * len(special)), replace=False)
    for i, q in enumerate(pos):
        x[q // C, q % C] = special[i % len(special)]
    if R > 1:
        x[R // 2, :] = 0.0
    if C > 1:
        x[:, C // 2] = 0.0
    q = int(rng.integers(0, n))
    if (R > 1 and q // C == R // 2) or (C > 1 and q % C == C // 2):
        q = 0
    x[q // C, q % C] = np.nan                                                         # one NaN: it must win
    x[:, C:] = np.nan
    return x


def prefill(n, kind):
    """uint32 [n]: zeros, or bit patterns of 0.25 .. 12.25 (above some of the maxima, below others)"""
    if kind == 'zero':
        return np.zeros(n, np.uint32)
    return (0.25 + 2.0 * (np.arange(n) % 7)).astype(np.float32).view(np.uint32)


def expected(x, C, pre_rows, pre_cols):
    """max(prefill, bits(|x|)) over the rows / columns of x[:, :C], as uint32"""
    bits = np.ascontiguousarray(x[:, :C]).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.maximum(pre_rows, bits.max(1)), np.maximum(pre_cols, bits.max(0))


def run(c):
    """one call of nabu_pk_amax -> the two whole destination buffers (uint32; None where not asked for)"""
    import torch
    from nabu_amd import ops
    R, C, ld, mode, pre = c
    x = torch.from_numpy(source(R, C, ld)).cuda()
    bufs = []
    for n, want in ((R, mode != 'cols'), (C, mode != 'rows')):
        if not want:
            bufs.append(None)
            continue
        host = np.full(GUARD + n + PAD + GUARD, SENTINEL, np.uint32)
        host[GUARD:GUARD + n] = prefill(n, pre)
        bufs.append(torch.from_numpy(host.view(np.int32)).cuda())
    ops.pk_amax(x, None if bufs[0] is None else bufs[0][GUARD:], None if bufs[1] is None else bufs[1][GUARD:], R, C, ld)
    torch.cuda.synchronize()
    return [None if b is None else b.cpu().numpy().view(np.uint32) for b in bufs]


# The pair form (two sources, shared row maxima) is internal: through the f16x3 BLSTM layer.  (B, T, D, H): the two
# small shapes with D = 40 (the first-layer path) and D = 128 (the packed-input path); below 2048 frames the layer
# computes f16x3 requests on bf16 planes, which take no maxima, so the same two inputs follow at 2048 frames, where
# the maxima kernels run.  Every shape in the automatic mode, in the stepwise mode (no persistent launch: the forward
# call measures the x maxima it keeps by itself) and with the two passes in DIFFERENT modes on one reserve (the reserve
# tag admits that: what the backward pass finds at res_axT_off may not depend on the forward call's mode).
LAYER_SHAPES = ((3, 5, 40, 64), (3, 5, 128, 64), (8, 256, 40, 128), (8, 256, 128, 128))
LAYER_KEYS = ('out', 'dx', 'fw_kernel', 'fw_bias', 'bw_kernel', 'bw_bias')


def layer_cases():
    return [(B, T, D, H, mode) for (B, T, D, H) in LAYER_SHAPES for mode in ('auto', 'stepwise', 'stepwise+auto', 'auto+stepwise')]


def layer_id(c):
    return 'blstm-%dx%dx%dx%d-%s' % c


def run_layer(c):
    """forward and backward of one f16x3 BLSTM layer -> {key: float32 array} (LAYER_KEYS)"""
    import torch
    from nabu_amd import ops
    B, T, D, H, mode = c
    rng = np.random.default_rng(B * T + D + H)
    lens = np.full(B, T)
    lens[-1] = max(1, T - 2)
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    for b in range(B):
        x[b, lens[b]:] = 0
    p = {k: (0.2 * rng.standard_normal(s)).astype(np.float32)
         for k, s in (('fw_kernel', (D + H, 4 * H)), ('fw_bias', (4 * H,)), ('bw_kernel', (D + H, 4 * H)), ('bw_bias', (4 * H,)))}
    dout = rng.standard_normal((B, T, 2 * H)).astype(np.float32)
    modes = [ops.LSTM_AUTO if m == 'auto' else ops.LSTM_STEPWISE for m in (mode.split('+') * 2)[:2]]      # forward, backward
    plan, bplan = [ops.BlstmPlan(B, T, D, H, int(lens.max()), m, 'f16x3') for m in modes]
    assert plan.reserve_bytes == bplan.reserve_bytes
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    pd = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    out = torch.full((B, T, 2 * H), float('nan'), device='cuda')
    reserve = torch.full((plan.reserve_bytes,), 0x7F, dtype=torch.uint8, device='cuda')   # (what no pass wrote reads as 3.4e38)
    ops.blstm_fwd(plan, xd, ld, pd['fw_kernel'], pd['fw_bias'], pd['bw_kernel'], pd['bw_bias'], out, reserve)
    dx = torch.full((B, T, D), float('nan'), device='cuda')
    g = {k: torch.full(v.shape, float('nan'), device='cuda') for k, v in pd.items()}
    ops.blstm_bwd(bplan, xd, ld, pd['fw_kernel'], pd['bw_kernel'], out, torch.from_numpy(dout).cuda(), reserve, dx,
                  g['fw_kernel'], g['fw_bias'], g['bw_kernel'], g['bw_bias'])
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in g.items()}
    res['out'], res['dx'] = out.cpu().numpy(), dx.cpu().numpy()
    return res


def main(argv):
    out = {}
    for c in layer_cases():
        for k, v in run_layer(c).items():
            out[layer_id(c) + '/' + k] = v
    for c in cases():
        for name, buf in zip(('rows', 'cols'), run(c)):
            if buf is not None:
                out[case_id(c) + '/' + name] = buf
    np.savez(argv[0], **out)
    print('PK AMAX CHILD OK %d cases' % len(cases()))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
