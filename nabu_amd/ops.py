"""Typed Python wrappers over the C ABI (one function per entry point of
include/nabu_hip.h).  Tensors are torch CUDA tensors used as device-memory
handles; all arithmetic happens inside libnabu_hip.so."""
import collections
import ctypes

import numpy as np
import torch

from . import _hip
from ._hip import ptr, stream, check, Workspace

LSTM_AUTO, LSTM_STEPWISE, LSTM_PERSISTENT = 0, 1, 2
NABU_EUNSUP = -2       # include/nabu_hip.h: shape not supported by the requested kernel


def _f32(t, name):
    if t.dtype != torch.float32:
        raise _hip.NabuHipError('%s must be float32, got %s' % (name, t.dtype))
    return t


def gemm(a, b, c, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, bias=None,
         M=None, N=None, K=None, lda=None, ldb=None, ldc=None,
         kseg=0, a_seg=0, b_seg=0, precision='default'):
    """c = alpha*op(a)@op(b) + beta*c + bias on 2-D row-major tensors (or raw
    views when M/N/K/ld* are given explicitly).  precision: 'default' | 'f32' | 'bf16' |
    'bf16x3' | 'bf16x6' (include/nabu_hip.h, nabu_gemm_ex)."""
    L = _hip.lib()
    if M is None:
        M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
        N = b.shape[0] if trans_b else b.shape[1]
        lda, ldb, ldc = a.stride(0), b.stride(0), c.stride(0)
    ws_bytes = L.nabu_gemm_ws_bytes(M, N, K)
    ws = Workspace.get(ws_bytes, c.device, 'gemm') if ws_bytes else None
    check(L.nabu_gemm_ex(_hip.GEMM_PRECISIONS[precision], int(trans_a), int(trans_b), M, N, K, alpha,
                         a.data_ptr(), lda, b.data_ptr(), ldb, beta, c.data_ptr(), ldc,
                         bias.data_ptr() if bias is not None else None, kseg, a_seg, b_seg,
                         ptr(ws), ws_bytes, stream()), 'nabu_gemm_ex')
    return c


def gemm2(a, b, a2, b2, c, beta=0.0, bias=None):
    """c = [a | a2] @ [b ; b2] + beta*c + bias for M <= 64 rows in one launch (nabu_gemm2_f32); a2/b2 may be None"""
    L = _hip.lib()
    M, K1 = a.shape
    N = b.shape[1]
    K2 = a2.shape[1] if a2 is not None else 0
    ws_bytes = L.nabu_gemm2_ws_bytes(M, N, K1, K2)
    ws = Workspace.get(ws_bytes, c.device, 'gemm2')
    check(L.nabu_gemm2_f32(M, N, K1, ptr(a), a.stride(0), ptr(b), b.stride(0), K2, ptr(a2),
                           a2.stride(0) if a2 is not None else 0, ptr(b2), b2.stride(0) if b2 is not None else 0,
                           beta, ptr(c), c.stride(0), ptr(bias), ptr(ws), ws_bytes, stream()), 'nabu_gemm2_f32')
    return c


class PackedOperand(object):
    """An fp32 matrix converted to the packed plane layout of gemm_pk.hip (include/nabu_hip.h, nabu_pk_pack):
    `rows` = the operand's M (or N) index, `K` = the reduction length.  planes = 3 / 1: bf16 planes; planes = 2:
    the scaled fp16 planes of f16x3, with `amax` = the bit patterns of the packed rows' largest magnitudes
    (pk_pack measures them unless told a bound)."""

    def __init__(self, rows, K, planes, device):
        L = _hip.lib()
        self.rows, self.K, self.planes = rows, K, planes
        self.rows_pad = L.nabu_pk_rows_pad(rows)
        self.nkb = L.nabu_pk_kblocks(K, planes)
        self.buf = torch.empty(L.nabu_pk_bytes(rows, K, planes), dtype=torch.uint8, device=device)
        self.amax = torch.zeros(self.rows_pad, dtype=torch.int32, device=device) if planes == 2 else None

    def kb_ptr(self, kb):
        return self.buf.data_ptr() + kb * self.planes * self.rows_pad * 32

    def row_ptr(self, row):
        return self.buf.data_ptr() + row * 32


def pk_amax(src, rows=None, cols=None, R=None, C=None, ld=None):
    """atomic maxima (bit patterns of |x|) of the rows / columns of the 2-D fp32 tensor `src` into the int32 device
    arrays `rows` [>= R] / `cols` [>= C], which the caller zeroed or seeded (nabu_pk_amax)"""
    if R is None:
        R, C = src.shape
        ld = src.stride(0)
    check(_hip.lib().nabu_pk_amax(src.data_ptr(), ld, R, C, ptr(rows), ptr(cols), stream()), 'nabu_pk_amax')


def pk_pack(dst, src, transposed=False, row_off=0, kb_off=0, fill_rows=None, fill_kb=None, period=0, shift=0,
            R=None, C=None, ld=None, bound=None, measure=True):
    """write the 2-D fp32 tensor `src` into the packed operand `dst` (rows / k-blocks beyond the source are zero).
    f16x3 operands (dst.planes == 2): the row maxima of the packed rows are measured first (`measure`; they
    accumulate when several sources share packed rows along k) or set to the a-priori `bound`."""
    if R is None:
        R, C = src.shape
        ld = src.stride(0)
    rows, kred = (C, R) if transposed else (R, C)
    if fill_rows is None:
        fill_rows = dst.rows_pad - row_off if row_off + rows >= dst.rows else rows
    if fill_kb is None:
        fill_kb = dst.nkb - kb_off if kb_off + (kred + 15) // 16 >= (dst.K + 15) // 16 else (kred + 15) // 16
    if dst.planes == 2:
        L = _hip.lib()
        am = dst.amax[row_off:]
        if bound is not None:
            check(L.nabu_pk_amax_fill(ptr(am), rows, float(bound), stream()), 'nabu_pk_amax_fill')
        elif measure:
            if kb_off == 0:        # a fresh measurement of these rows (the maxima accumulate only along k: kb_off > 0)
                am[:rows].zero_()
            check(L.nabu_pk_amax(src.data_ptr(), ld, R, C, None if transposed else ptr(am), ptr(am) if transposed else None,
                                 stream()), 'nabu_pk_amax')
        check(L.nabu_pk_pack_f16(int(transposed), src.data_ptr(), ld, R, C, ptr(dst.buf), dst.rows_pad, row_off, kb_off,
                                 fill_rows, fill_kb, period, shift, ptr(dst.amax), stream()), 'nabu_pk_pack_f16')
        return dst
    check(_hip.lib().nabu_pk_pack(dst.planes, int(transposed), src.data_ptr(), ld, R, C, ptr(dst.buf), dst.rows_pad,
                                  row_off, kb_off, fill_rows, fill_kb, period, shift, stream()), 'nabu_pk_pack')
    return dst


def gemm_pk(a, b, c, planes=None, alpha=1.0, beta=0.0, bias=None, c2=None, n_split=0, bias2=None, M=None, N=None,
            nkb=None, a_ptrs=None, b_ptrs=None, cs=None, c2s=None, a_amax=None, b_amax=None, direct=False):
    """c[M,N] = alpha * a·b^T + beta*c + bias over packed operands (nabu_gemm_pk); batched form through
    a_ptrs / b_ptrs / cs (lists of raw pointers / tensors, <= 2 entries)"""
    L = _hip.lib()
    planes = planes or min(a.planes, b.planes)
    d = _hip.PkGemmDesc()
    d.size = ctypes.sizeof(_hip.PkGemmDesc)
    d.planes = planes
    d.M = a.rows if M is None else M
    d.N = b.rows if N is None else N
    d.nkb = L.nabu_pk_kblocks(a.K, planes) if nkb is None else nkb
    cs = cs or [c]
    d.nbatch = len(cs)
    for i in range(d.nbatch):
        d.A[i] = a_ptrs[i] if a_ptrs else a.buf.data_ptr()
        d.B[i] = b_ptrs[i] if b_ptrs else b.buf.data_ptr()
        d.C[i] = ptr(cs[i])
        d.C2[i] = ptr(c2s[i]) if c2s else ptr(c2)
    d.a_rows_pad, d.b_rows_pad, d.a_planes, d.b_planes = a.rows_pad, b.rows_pad, a.planes, b.planes
    d.ldc, d.n_split = cs[0].stride(0), n_split
    d.bias, d.bias2 = ptr(bias), ptr(bias2)
    d.alpha, d.beta = alpha, beta
    d.direct = int(direct)            # 0 promoted accumulation, 1 direct chain, 2 by rounding count (nabu_hip.h)
    if planes == 2:
        for i in range(d.nbatch):
            d.a_amax[i] = (a_amax[i] if a_amax else a.amax.data_ptr())
            d.b_amax[i] = (b_amax[i] if b_amax else b.amax.data_ptr())
    ws_bytes = L.nabu_gemm_pk_ws_bytes(ctypes.byref(d))
    ws = Workspace.get(ws_bytes, cs[0].device, 'gemm') if ws_bytes else None
    check(L.nabu_gemm_pk(ctypes.byref(d), ptr(ws), ws_bytes, stream()), 'nabu_gemm_pk')
    return c


def set_gemm_precision(precision):
    """process default of every GEMM that does not name a precision ('f32' | 'bf16' | 'bf16x3' | 'bf16x6' | 'f16x3')"""
    check(_hip.lib().nabu_gemm_set_default_precision(_hip.GEMM_PRECISIONS[precision]), 'nabu_gemm_set_default_precision')


def get_gemm_precision():
    code = _hip.lib().nabu_gemm_get_default_precision()
    return [k for k, v in _hip.GEMM_PRECISIONS.items() if v == code][0]


def colsum(a, out, beta=0.0):
    """out[n] = beta*out[n] + sum_m a[m,n] for a 2-D row-major tensor."""
    L = _hip.lib()
    M, N = a.shape
    ws_bytes = L.nabu_colsum_ws_bytes(M, N)
    ws = Workspace.get(ws_bytes, a.device, 'gemm')
    check(L.nabu_colsum_f32(M, N, ptr(a), a.stride(0), beta, ptr(out), ptr(ws), ws_bytes, stream()),
          'nabu_colsum_f32')
    return out


def linear_bwd(x, dy, w, dw, db, dx=None):
    """All gradients of y = x @ w + b for a narrow output (w.shape[1] <= 64) from one pass over x and dy
    (nabu_linear_bwd_f32): dw = x^T dy and db = colsum(dy) overwritten, dx = dy w^T when dx is given.  Returns False,
    with nothing written, when the shape is not supported there (NABU_EUNSUP): the caller then makes the three calls."""
    L = _hip.lib()
    M, K = x.shape
    N = w.shape[1]
    if not (dw.is_contiguous() and x.stride(1) == 1 and dy.stride(1) == 1 and w.stride(1) == 1 and
            (dx is None or dx.stride(1) == 1)):
        return False
    ws_bytes = L.nabu_linear_bwd_ws_bytes(M, K, N)
    ws = Workspace.get(ws_bytes, x.device, 'gemm')
    rc = L.nabu_linear_bwd_f32(M, K, N, _f32(x, 'x').data_ptr(), x.stride(0), _f32(dy, 'dy').data_ptr(), dy.stride(0),
                               _f32(w, 'w').data_ptr(), w.stride(0), _f32(dx, 'dx').data_ptr() if dx is not None else None,
                               dx.stride(0) if dx is not None else 0, ptr(_f32(dw, 'dw')), ptr(_f32(db, 'db')),
                               ptr(ws), ws_bytes, stream())
    if rc == NABU_EUNSUP:
        return False
    check(rc, 'nabu_linear_bwd_f32')
    return True


class BlstmPlan(object):
    """Shape descriptor + buffers of one BLSTM layer call (plain cell: the nabu_blstm_* entry points)."""
    ENTRY, WS_TAG, LAYER_NORM = 'nabu_blstm', 'blstm', False

    def __init__(self, B, T, D, H, max_len, mode=LSTM_AUTO, gemm_precision='default', x_bound=0.0, fwd_only=False,
                 recurrent_precision='default', out_stack=0):
        """x_bound > 0: |x| <= x_bound is guaranteed (the previous layer's LSTM outputs) — the f16x3 packs of x skip their
        measuring pass; fwd_only: no backward pass follows (validation): the reserve holds the activations only;
        recurrent_precision 'f32': the exact-fp32 recurrent kernels (include/nabu_hip.h, nabu_blstm_desc)"""
        import os
        # (NABU_DESC_V1=1: the 32-byte ABI-version-1 descriptor — A/B runs against a library built before round 5)
        v1 = os.environ.get('NABU_DESC_V1') == '1' and not self.LAYER_NORM
        if self.LAYER_NORM:
            x_bound, recurrent_precision, out_stack = 0.0, 'default', 0
        self.desc = _hip.BlstmDesc(32 if v1 else ctypes.sizeof(_hip.BlstmDesc), B, T, D, H, int(max_len), mode,
                                   _hip.GEMM_PRECISIONS[gemm_precision], float(x_bound),
                                   _hip.BLSTM_FWD_ONLY if fwd_only else 0, _hip.REC_PRECISIONS[recurrent_precision],
                                   int(out_stack), None, None, None, None, None)
        L = _hip.lib()
        # packed companions (ABI version 3): sizes of x_pk_rows, x_pk_cols, hT_pk, out_pk_rows, out_pk_cols for this layer
        # (0 = the layer would not use that companion); the buffers themselves are attached by the caller (set_companions)
        pkb = (ctypes.c_size_t * 5)()
        self.pk_bytes = [0] * 5
        if not (v1 or self.LAYER_NORM) and L.nabu_blstm_pk_bytes(ctypes.byref(self.desc), pkb) == 0:
            self.pk_bytes = [int(v) for v in pkb]
        self._keep = []
        self.reserve_bytes = getattr(L, self.ENTRY + '_reserve_bytes')(ctypes.byref(self.desc))
        self.ws_bytes = getattr(L, self.ENTRY + '_ws_bytes')(ctypes.byref(self.desc))
        if self.reserve_bytes == 0:
            raise _hip.NabuHipError('%s: unsupported shape B=%d T=%d D=%d H=%d mode=%d: %s' % (
                self.ENTRY, B, T, D, H, mode, L.nabu_last_error().decode()))


class BlstmLnPlan(BlstmPlan):
    """... of one layer-normalised BLSTM layer call (nabu_blstm_ln_*): the same descriptor, sized by those entry points,
    which do not look at x_bound, recurrent_precision, out_stack and the companions (left 0).  LSTM_PERSISTENT is refused
    there, with the reason."""
    ENTRY, WS_TAG, LAYER_NORM = 'nabu_blstm_ln', 'blstm_ln', True


def blstm_set_companions(plan, x_pk=None, out_pk=None, hT_pk=None):
    """attach packed companions to a plan (include/nabu_hip.h, nabu_blstm_desc ABI version 3): x_pk / out_pk = (rows, cols)
    uint8 tensors of plan.pk_bytes[0:2] / [3:5] bytes, hT_pk one tensor of plan.pk_bytes[2] bytes, each zero-filled once
    by its owner.  The plan keeps them alive."""
    d = plan.desc
    if x_pk is not None:
        assert x_pk[0].numel() == plan.pk_bytes[0] and x_pk[1].numel() == plan.pk_bytes[1]
        d.x_pk_rows, d.x_pk_cols = x_pk[0].data_ptr(), x_pk[1].data_ptr()
    if out_pk is not None:
        assert out_pk[0].numel() == plan.pk_bytes[3] and out_pk[1].numel() == plan.pk_bytes[4]
        d.out_pk_rows, d.out_pk_cols = out_pk[0].data_ptr(), out_pk[1].data_ptr()
    if hT_pk is not None:
        assert hT_pk.numel() == plan.pk_bytes[2]
        d.hT_pk = hT_pk.data_ptr()
    plan._keep += [t for t in (x_pk or ()) + (out_pk or ()) + ((hT_pk,) if hT_pk is not None else ())]


def blstm_emits_packed(plan, out_pk=False, hT_pk=False):
    """which companions nabu_blstm_fwd's recurrent kernel writes itself (bit 0 rows, 1 transposed, 2 h^T): of those
    attached to `plan`, plus the out_pk / hT_pk ones it would name.  The query reads the descriptor's pointers for null
    only, so a would-be companion is named by a placeholder for its duration: the caller allocates only what is written."""
    d = plan.desc
    attached = d.out_pk_rows, d.out_pk_cols, d.hT_pk
    if out_pk:
        d.out_pk_rows, d.out_pk_cols = d.out_pk_rows or 1, d.out_pk_cols or 1
    if hT_pk:
        d.hT_pk = d.hT_pk or 1
    try:
        return int(_hip.lib().nabu_blstm_emits_packed(ctypes.byref(d)))
    finally:
        d.out_pk_rows, d.out_pk_cols, d.hT_pk = attached


def _blstm_call(plan, part, x, *args, **kw):
    """<plan.ENTRY>_<part>(descriptor, x, args..., workspace, its size, stream): tensors (or None) go as pointers, anything
    else as it is.  profile = 'fwd' | 'bwd': the call runs a plain recurrence — BEFORE_RECURRENT and the PROFILER fire."""
    profile = kw.get('profile')
    name = '%s_%s' % (plan.ENTRY, part)
    ws = Workspace.get(plan.ws_bytes, x.device, plan.WS_TAG)
    if profile and BEFORE_RECURRENT[0] is not None:
        BEFORE_RECURRENT[0]()
    if profile and PROFILER is not None:
        PROFILER.arm(profile, plan)
    argv = [ptr(a) if a is None or torch.is_tensor(a) else a for a in (_f32(x, 'x'),) + args]
    check(getattr(_hip.lib(), name)(ctypes.byref(plan.desc), *(argv + [ptr(ws), plan.ws_bytes, stream()])), name)
    if profile and PROFILER is not None:
        PROFILER.disarm()


def blstm_fwd(plan, x, lens_dev, k_fw, b_fw, k_bw, b_bw, out, reserve):
    _blstm_call(plan, 'fwd', x, lens_dev, k_fw, b_fw, k_bw, b_bw, out, reserve, profile='fwd')
    return out


def blstm_bwd(plan, x, lens_dev, k_fw, k_bw, out, d_out, reserve, d_x, dk_fw, db_fw, dk_bw, db_bw):
    _blstm_call(plan, 'bwd', x, lens_dev, k_fw, k_bw, out, d_out, reserve, d_x, dk_fw, db_fw, dk_bw, db_bw, profile='bwd')
    return d_x


def blstm_bwd_data(plan, x, lens_dev, k_fw, k_bw, out, d_out, reserve, d_x, db_fw, db_bw):
    """first half of blstm_bwd (nabu_blstm_bwd_data): recurrence backward, bias gradients, d_x; dz stays in `reserve`"""
    _blstm_call(plan, 'bwd_data', x, lens_dev, k_fw, k_bw, out, d_out, reserve, d_x, db_fw, db_bw, profile='bwd')
    return d_x


def blstm_bwd_weights(plan, x, lens_dev, out, reserve, dk_fw, dk_bw):
    """second half (nabu_blstm[_ln]_bwd_weights): the kernel gradients from the dz the data half left in `reserve`"""
    _blstm_call(plan, 'bwd_weights', x, lens_dev, out, reserve, dk_fw, dk_bw)


LN_SCOPES = ('input', 'transform', 'forget', 'output', 'state')    # the norm scopes of LayerNormBasicLSTMCell, in ABI order


def blstm_ln_params(gamma, beta, dgamma=None, dbeta=None):
    """nabu_blstm_ln_params from [fw, bw] lists of five [H] tensors each (LN_SCOPES order); the gradients for a backward call"""
    p = _hip.BlstmLnParams(ctypes.sizeof(_hip.BlstmLnParams), 0)
    for d in range(2):
        for k in range(5):
            p.gamma[d][k], p.beta[d][k] = ptr(_f32(gamma[d][k], 'gamma')), ptr(_f32(beta[d][k], 'beta'))
            if dgamma is not None:
                p.dgamma[d][k], p.dbeta[d][k] = ptr(_f32(dgamma[d][k], 'dgamma')), ptr(_f32(dbeta[d][k], 'dbeta'))
    return p


def blstm_ln_fwd(plan, x, lens_dev, k_fw, k_bw, gamma, beta, out, reserve):
    _blstm_call(plan, 'fwd', x, lens_dev, k_fw, k_bw, ctypes.byref(blstm_ln_params(gamma, beta)), out, reserve)
    return out


def blstm_ln_bwd(plan, x, lens_dev, k_fw, k_bw, gamma, beta, out, d_out, reserve, d_x, dk_fw, dk_bw, dgamma, dbeta):
    _blstm_call(plan, 'bwd', x, lens_dev, k_fw, k_bw, ctypes.byref(blstm_ln_params(gamma, beta, dgamma, dbeta)), out, d_out,
                reserve, d_x, dk_fw, dk_bw)
    return d_x


def blstm_ln_bwd_data(plan, x, lens_dev, k_fw, k_bw, gamma, beta, out, d_out, reserve, d_x, dgamma, dbeta):
    """first half of blstm_ln_bwd: recurrence backwards, the norm-parameter gradients, d_x; dz stays in `reserve`"""
    _blstm_call(plan, 'bwd_data', x, lens_dev, k_fw, k_bw, ctypes.byref(blstm_ln_params(gamma, beta, dgamma, dbeta)), out,
                d_out, reserve, d_x)
    return d_x


blstm_ln_bwd_weights = blstm_bwd_weights     # (the plan names the family)


def pad_time(x, Tp):
    B, T, F = x.shape
    y = torch.empty((B, Tp, F), dtype=x.dtype, device=x.device)
    check(_hip.lib().nabu_pad_time_f32(B, T, Tp, F, ptr(x), ptr(y), stream()), 'nabu_pad_time_f32')
    return y


def unpad_time(y, T):
    B, Tp, F = y.shape
    x = torch.empty((B, T, F), dtype=y.dtype, device=y.device)
    check(_hip.lib().nabu_unpad_time_f32(B, T, Tp, F, ptr(y), ptr(x), stream()), 'nabu_unpad_time_f32')
    return x


def ctc_loss_grad(logits, logit_len_dev, labels_dev, label_len_dev, grad_scale):
    """Returns (nll [B], dlogits [B,T,C], status [1] int32) — all on device."""
    L = _hip.lib()
    B, T, C = logits.shape
    Lmax = labels_dev.shape[1]
    nll = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    status = torch.empty(1, dtype=torch.int32, device=logits.device)
    ws_bytes = L.nabu_ctc_ws_bytes(B, T, Lmax)
    ws = Workspace.get(ws_bytes, logits.device, 'ctc')
    check(L.nabu_ctc_loss_grad(B, T, C, Lmax, ptr(_f32(logits, 'logits')), ptr(logit_len_dev),
                               ptr(labels_dev), ptr(label_len_dev), grad_scale, ptr(nll), ptr(dlogits),
                               ptr(status), ptr(ws), ws_bytes, stream()), 'nabu_ctc_loss_grad')
    return nll, dlogits, status


def ctc_align(logits, logit_len_dev, labels_dev, label_len_dev, raise_on_status=False):
    """Forced alignment (nabu_ctc_align): returns (state [B,T] int32, seg [B,Lmax,2] int32, conf [B,Lmax],
    score [B], status [1] int32) — all on device.  status is 1+b for the first utterance b without a valid alignment;
    raise_on_status: read it back (a synchronisation) and raise what the CTC loss raises for such an utterance."""
    L = _hip.lib()
    B, T, C = logits.shape
    Lmax = labels_dev.shape[1]
    dev = logits.device
    state = torch.empty((B, T), dtype=torch.int32, device=dev)
    seg = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    conf = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = L.nabu_ctc_align_ws_bytes(B, T, Lmax)
    ws = Workspace.get(ws_bytes, dev, 'ctc_align')
    check(L.nabu_ctc_align(B, T, C, Lmax, ptr(_f32(logits, 'logits')), ptr(logit_len_dev),
                           ptr(labels_dev) if Lmax else None, ptr(label_len_dev), ptr(state), ptr(seg), ptr(conf),
                           ptr(score), ptr(status), ptr(ws), ws_bytes, stream()), 'nabu_ctc_align')
    if raise_on_status:
        code = int(status.item())
        if code:
            from nabu_amd.neuralnetworks.trainers import loss_functions
            raise loss_functions.ctc_status_error(code)
    return state, seg, conf, score, status


def transducer_loss_grad(f, g, enc_len_dev, labels_dev, label_len_dev, grad_scale):
    """Transducer loss with the additive joint (nabu_transducer_loss_grad): f [B,T,C], g [B,U1,C], labels [B,>=U1-1]
    int32 (None when U1 = 1).  Returns (nll [B], df [B,T,C], dg [B,U1,C], status [1] int32) — all on device."""
    L = _hip.lib()
    B, T, C = f.shape
    U1 = g.shape[1]
    if g.shape[0] != B or g.shape[2] != C:
        raise _hip.NabuHipError('transducer_loss_grad: f %s and g %s do not agree' % (tuple(f.shape), tuple(g.shape)))
    if labels_dev is not None and labels_dev.stride(1) != 1:
        raise _hip.NabuHipError('transducer_loss_grad: labels must be contiguous in their rows')
    dev = f.device
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    df, dg = torch.empty_like(f), torch.empty_like(g)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = L.nabu_transducer_ws_bytes(B, T, U1)
    ws = Workspace.get(ws_bytes, dev, 'transducer')
    check(L.nabu_transducer_loss_grad(B, T, U1, C, ptr(_f32(f, 'f')), ptr(_f32(g, 'g')), ptr(enc_len_dev),
                                      ptr(labels_dev) if labels_dev is not None and labels_dev.numel() else None,
                                      labels_dev.stride(0) if labels_dev is not None and labels_dev.numel() else 0,
                                      ptr(label_len_dev), grad_scale, ptr(nll), ptr(df), ptr(dg), ptr(status), ptr(ws),
                                      ws_bytes, stream()), 'nabu_transducer_loss_grad')
    return nll, df, dg, status


def transducer_align(f, g, enc_len_dev, labels_dev, label_len_dev, raise_on_status=False):
    """Forced alignment with the transducer (nabu_transducer_align), operands as in transducer_loss_grad.  Returns
    (state [B,T] int32, frame [B,U1-1] int32, conf [B,U1-1], score [B], status [1] int32) — all on device.  status is
    1+b for the first utterance b the loss would reject; raise_on_status: read it back (a synchronisation) and raise
    what the transducer loss raises for such an utterance."""
    L = _hip.lib()
    B, T, C = f.shape
    U1 = g.shape[1]
    if g.shape[0] != B or g.shape[2] != C:
        raise _hip.NabuHipError('transducer_align: f %s and g %s do not agree' % (tuple(f.shape), tuple(g.shape)))
    if labels_dev is not None and labels_dev.stride(1) != 1:
        raise _hip.NabuHipError('transducer_align: labels must be contiguous in their rows')
    dev = f.device
    state = torch.empty((B, T), dtype=torch.int32, device=dev)
    frame = torch.empty((B, U1 - 1), dtype=torch.int32, device=dev)
    conf = torch.empty((B, U1 - 1), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = L.nabu_transducer_align_ws_bytes(B, T, U1)
    ws = Workspace.get(ws_bytes, dev, 'transducer_align')
    has_labels = labels_dev is not None and labels_dev.numel()
    check(L.nabu_transducer_align(B, T, U1, C, ptr(_f32(f, 'f')), ptr(_f32(g, 'g')), ptr(enc_len_dev),
                                  ptr(labels_dev) if has_labels else None, labels_dev.stride(0) if has_labels else 0,
                                  ptr(label_len_dev), ptr(state), ptr(frame) if U1 > 1 else None,
                                  ptr(conf) if U1 > 1 else None, ptr(score), ptr(status), ptr(ws), ws_bytes, stream()),
          'nabu_transducer_align')
    if raise_on_status:
        code = int(status.item())
        if code:
            from nabu_amd.neuralnetworks.trainers import loss_functions
            raise loss_functions.transducer_status_error(code)
    return state, frame, conf, score, status


def transducer_greedy_step(step, f, g_row, enc_len_dev, t_pos, out_len, ids, emit, last_id, score):
    """One lock-step iteration of the greedy transducer search (nabu_transducer_greedy_step), in place on the search
    state t_pos / out_len / last_id / score [B], ids [B,S]; emit [B] says which rows emitted a label.  step = 0 starts
    a search: the kernel sets the state up itself."""
    B, T, C = f.shape
    check(_hip.lib().nabu_transducer_greedy_step(B, T, C, ids.shape[1], step, ptr(_f32(f, 'f')), ptr(_f32(g_row, 'g_row')),
                                                 ptr(enc_len_dev), ptr(t_pos), ptr(out_len), ptr(ids), ptr(emit),
                                                 ptr(last_id), ptr(_f32(score, 'score')), stream()),
          'nabu_transducer_greedy_step')


class TransducerBeamState(object):
    """the state of nabu_transducer_beam_step: the beam ids [B,W,S], out_len, score [B,W]; parent, emit, last_id [B,W] for
    the prediction network; the finals fin_ids [B,W,S], fin_len, fin_score [B,W] (best first); the workspace.  Nothing
    is cleared: step 0 sets everything up."""

    def __init__(self, B, W, S, device):
        self.B, self.W, self.S = int(B), int(W), int(S)

        def i32(*shape):
            return torch.empty(shape, dtype=torch.int32, device=device)

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=device)
        self.ids, self.out_len, self.score = i32(B, W, S), i32(B, W), f32(B, W)
        self.parent, self.emit, self.last_id = i32(B, W), i32(B, W), i32(B, W)
        self.fin_ids, self.fin_len, self.fin_score = i32(B, W, S), i32(B, W), f32(B, W)
        self.ws = torch.empty(max(self.ws_bytes(2), 16), dtype=torch.uint8, device=device)

    def ws_bytes(self, C):
        return _hip.lib().nabu_transducer_beam_ws_bytes(self.B, self.W, C, self.S)


def transducer_beam_state(B, W, S, device):
    """the tensors and the workspace of a beam search over B utterances with W slots of at most S labels each"""
    return TransducerBeamState(B, W, S, device)


def transducer_beam_step(step, f, g_rows, enc_len_dev, state):
    """One iteration of the alignment-length synchronous beam search (nabu_transducer_beam_step), in place on `state`:
    f [B,T,C], g_rows [B,W,C] (or [B*W,C]) the prediction logits of the hypothesis in each slot.  step = 0 starts a
    search."""
    B, T, C = f.shape
    st = state
    if st.B != B or g_rows.numel() != B * st.W * C:
        raise _hip.NabuHipError('transducer_beam_step: f %s, g_rows %s and a state of [%d,%d] slots do not agree'
                                % (tuple(f.shape), tuple(g_rows.shape), st.B, st.W))
    if g_rows.dtype != torch.float32 or not g_rows.is_contiguous():
        raise _hip.NabuHipError('transducer_beam_step: g_rows must be contiguous float32')
    need = st.ws_bytes(C)
    if st.ws.numel() < need:
        st.ws = torch.empty(need, dtype=torch.uint8, device=f.device)
    check(_hip.lib().nabu_transducer_beam_step(B, T, C, st.S, st.W, step, ptr(_f32(f, 'f')), ptr(g_rows),
                                               ptr(enc_len_dev), ptr(st.ids), ptr(st.out_len), ptr(st.score),
                                               ptr(st.parent), ptr(st.emit), ptr(st.last_id), ptr(st.fin_ids),
                                               ptr(st.fin_len), ptr(st.fin_score), ptr(st.ws), st.ws.numel(), stream()),
          'nabu_transducer_beam_step')


def adam_clip_step(param, grad, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-8, clip=1.0, grad_scale=1.0):
    check(_hip.lib().nabu_adam_clip_step(param.numel(), ptr(param), ptr(grad), ptr(m), ptr(v), lr_t, b1, b2,
                                         eps, clip, grad_scale, stream()), 'nabu_adam_clip_step')


def adam_clip_step_from(param_out, src, grad, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-8, clip=1.0, grad_scale=1.0):
    """adam_clip_step with the parameter read from `src` (read-only, no overlap with param_out):
    param_out = src - lr_t * m / (sqrt(v) + eps) — the update of a weight-noise step from the clean parameters"""
    if src.numel() != param_out.numel():
        raise _hip.NabuHipError('adam_clip_step_from: src holds %d elements, param_out %d' % (src.numel(), param_out.numel()))
    check(_hip.lib().nabu_adam_clip_step_from(param_out.numel(), ptr(_f32(param_out, 'param_out')), ptr(_f32(src, 'src')),
                                              ptr(grad), ptr(m), ptr(v), lr_t, b1, b2, eps, clip, grad_scale, stream()),
          'nabu_adam_clip_step_from')


def clip_(g, clip=1.0):
    check(_hip.lib().nabu_clip_f32(g.numel(), ptr(g), clip, stream()), 'nabu_clip_f32')
    return g


def clip_accumulate(out, acc, g, clip=1.0):
    """out = clamp(g, +-clip) + acc (acc None: out = clamp(g, +-clip), nothing read but g); out may be acc or g
    (nabu_clip_accumulate_f32): one micro-batch of an accumulated update.  A None out or g reaches the entry point as
    NULL and is its argument error."""
    given = [(name, _f32(t, name)) for name, t in (('g', g), ('out', out), ('acc', acc)) if t is not None]
    n = given[0][1].numel() if given else 0
    for name, t in given:
        if t.numel() != n:
            raise _hip.NabuHipError('clip_accumulate: %s holds %d elements, %s %d' % (name, t.numel(), given[0][0], n))
    check(_hip.lib().nabu_clip_accumulate_f32(n, ptr(out), ptr(acc), ptr(g), clip, stream()), 'nabu_clip_accumulate_f32')
    return out


def adam_clip_step_acc(param_out, src, acc, g, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-8, clip=1.0, grad_scale=1.0):
    """adam_clip_step (src None) or adam_clip_step_from (src: the clean parameters) on the gradient
    acc + clamp(g, +-clip): the update of an accumulated step's last micro-batch (nabu_adam_clip_step_acc)"""
    for name, t in (('src', src), ('acc', acc), ('g', g)):
        if t is not None and t.numel() != param_out.numel():
            raise _hip.NabuHipError('adam_clip_step_acc: %s holds %d elements, param_out %d'
                                    % (name, t.numel(), param_out.numel()))
    check(_hip.lib().nabu_adam_clip_step_acc(param_out.numel(), ptr(_f32(param_out, 'param_out')), ptr(src),
                                             ptr(_f32(acc, 'acc')), ptr(_f32(g, 'g')), ptr(m), ptr(v), lr_t, b1, b2, eps,
                                             clip, grad_scale, stream()), 'nabu_adam_clip_step_acc')


def grad_norm_buffers(n, device):
    """(stats, ws) of grad_norm for a gradient of n elements: the four zeroed 32-bit words (float norm, float factor,
    int32 skipped, 0) and the workspace of the per-block partial sums"""
    ws_bytes = _hip.lib().nabu_grad_norm_ws_bytes(n)
    return (torch.zeros(4, dtype=torch.int32, device=device),
            torch.empty(max(ws_bytes, 8) // 8, dtype=torch.float64, device=device))


def grad_norm(g, acc, scale, max_norm, stats, ws):
    """stats = (norm, factor, skipped += norm not finite, 0) of the gradient scale * g, with acc of scale * (acc + g):
    norm = its L2 norm, summed in double in a fixed order, factor = scale * min(1, max_norm / norm) or NaN when the norm
    is NaN or inf (nabu_grad_norm_f32).  stats and ws come from grad_norm_buffers; nothing is read back."""
    if acc is not None and acc.numel() != g.numel():
        raise _hip.NabuHipError('grad_norm: acc holds %d elements, g %d' % (acc.numel(), g.numel()))
    if stats is not None and (stats.dtype != torch.int32 or stats.numel() != 4):
        raise _hip.NabuHipError('grad_norm: stats must be 4 int32 words (grad_norm_buffers)')
    check(_hip.lib().nabu_grad_norm_f32(g.numel(), ptr(_f32(g, 'g')), ptr(acc if acc is None else _f32(acc, 'acc')),
                                        scale, max_norm, ptr(stats), ptr(ws),
                                        0 if ws is None else ws.numel() * ws.element_size(), stream()),
          'nabu_grad_norm_f32')
    return stats


def read_grad_stats(stats):
    """(norm, factor, skipped) of a stats buffer of grad_norm; copies to the host, so it synchronises"""
    words = stats.cpu()
    f = words.view(torch.float32)
    return float(f[0]), float(f[1]), int(words[2])


def adam_scaled_step(param_out, src, acc, g, m, v, lr_t, b1, b2, eps, stats):
    """adam_clip_step (src None) / _from (src: the clean parameters) / _acc (acc: the sum of the earlier micro-batch
    gradients) without a clamp, on factor * g or factor * (acc + g) with factor = stats[1] read on the device; a NaN
    factor leaves m, v and the parameters alone (with src: param_out = src) (nabu_adam_scaled_step)"""
    for name, t in (('src', src), ('acc', acc), ('g', g)):
        if t is not None and t.numel() != param_out.numel():
            raise _hip.NabuHipError('adam_scaled_step: %s holds %d elements, param_out %d'
                                    % (name, t.numel(), param_out.numel()))
    check(_hip.lib().nabu_adam_scaled_step(param_out.numel(), ptr(_f32(param_out, 'param_out')), ptr(src), ptr(acc),
                                           ptr(_f32(g, 'g')), ptr(m), ptr(v), lr_t, b1, b2, eps, ptr(stats), stream()),
          'nabu_adam_scaled_step')


def dropout(x, keep_prob, seed, offset):
    y = torch.empty_like(x)
    check(_hip.lib().nabu_dropout_f32(x.numel(), ptr(x), ptr(y), keep_prob, seed, offset, stream()),
          'nabu_dropout_f32')
    return y


def sample_ids(logits, prob, seed, offset, teacher_ids):
    """scheduled-sampling choice of the next decoder input (ScheduledEmbeddingTrainingHelper)"""
    B, C = logits.shape
    out = torch.empty_like(teacher_ids)
    check(_hip.lib().nabu_sample_ids(B, C, ptr(logits), prob, seed, offset, ptr(teacher_ids), ptr(out), stream()),
          'nabu_sample_ids')
    return out


def gaussian_noise(x, stddev, seed, offset):
    y = torch.empty_like(x)
    check(_hip.lib().nabu_gaussian_noise_f32(x.numel(), ptr(x), ptr(y), stddev, seed, offset, stream()),
          'nabu_gaussian_noise_f32')
    return y


WEIGHT_NOISE_MAX_RANGES = 1024      # NABU_WEIGHT_NOISE_MAX_RANGES of include/nabu_hip.h


class WeightNoiseTable(object):
    """the range table of nabu_weight_noise_f32: [first_group, end_group) pairs in units of 4 elements, kept as the int32
    host array the call validates and as its device copy the kernel reads (uploaded once, here)"""

    def __init__(self, ranges, device):
        self.host = np.ascontiguousarray(np.asarray(list(ranges), np.int64).reshape(-1, 2).astype(np.int32))
        self.n = int(self.host.shape[0])
        self.dev = torch.from_numpy(self.host).to(device) if self.n else None


def weight_noise(param, clean, table, stddev, seed, offset):
    """in place: clean = param, then param += stddev * N(0, 1) inside the ranges of `table` (a WeightNoiseTable), with the
    values gaussian_noise draws for an array of param.numel() elements at (seed, offset) (nabu_weight_noise_f32)"""
    if clean.numel() != param.numel():
        raise _hip.NabuHipError('weight_noise: clean holds %d elements, param %d' % (clean.numel(), param.numel()))
    check(_hip.lib().nabu_weight_noise_f32(param.numel(), ptr(_f32(param, 'param')), ptr(_f32(clean, 'clean')),
                                           ptr(table.dev), table.host.ctypes.data if table.n else None, table.n,
                                           stddev, seed, offset, stream()), 'nabu_weight_noise_f32')
    return param


SPECAUG_MAX_MASKS = _hip.SPECAUG_MAX_MASKS       # masks of one kind per utterance (include/nabu_hip.h)


class SpecAugmentPolicy(collections.namedtuple('SpecAugmentPolicy', [
        'time_warp', 'time_masks', 'time_mask_width', 'time_mask_ratio', 'freq_masks', 'freq_mask_width',
        'feature_blocks'])):
    """what nabu_spec_augment_f32 does to every utterance (include/nabu_hip.h): the anchor's largest shift W, the
    number and the largest width of the time masks (a width is also capped at time_mask_ratio times the length) and of
    the frequency masks, and the number of equal column blocks a frequency mask repeats in"""
    __slots__ = ()

    def __new__(cls, time_warp=0, time_masks=0, time_mask_width=0, time_mask_ratio=1.0, freq_masks=0,
                freq_mask_width=0, feature_blocks=1):
        return super(SpecAugmentPolicy, cls).__new__(cls, int(time_warp), int(time_masks), int(time_mask_width),
                                                     float(time_mask_ratio), int(freq_masks), int(freq_mask_width),
                                                     int(feature_blocks))

    @property
    def on(self):
        """False: the policy draws nothing and changes nothing"""
        return self.time_warp > 0 or self.time_masks > 0 or self.freq_masks > 0

    @property
    def param_width(self):
        """ints per utterance of the parameter buffer: (c, c'), (t0, t) per time mask, (f0, f) per frequency mask"""
        return 2 + 2 * self.time_masks + 2 * self.freq_masks


def spec_augment(x, len_dev, policy, seed, offset, params=None):
    """SpecAugment of x [B, T, D] with the device lengths len_dev [B] at the stream (seed, offset); params: an int32
    [B, policy.param_width] device tensor that receives what was drawn, or None"""
    B, T, D = x.shape
    y = torch.empty_like(x)
    if params is not None and (params.dtype != torch.int32 or tuple(params.shape) != (B, policy.param_width)):
        raise _hip.NabuHipError('spec_augment: params must be int32 [%d, %d]' % (B, policy.param_width))
    if len_dev.dtype != torch.int32 or len_dev.numel() != B:
        raise _hip.NabuHipError('spec_augment: the lengths must be int32 [%d]' % B)
    d = _hip.SpecAugDesc(ctypes.sizeof(_hip.SpecAugDesc), B, T, D, policy.feature_blocks, policy.time_warp,
                         policy.time_masks, policy.time_mask_width, policy.freq_masks, policy.freq_mask_width,
                         policy.time_mask_ratio)
    check(_hip.lib().nabu_spec_augment_f32(ctypes.byref(d), ptr(_f32(x, 'x')), ptr(len_dev), ptr(y), ptr(params), seed,
                                           offset, stream()), 'nabu_spec_augment_f32')
    return y


def sum_(x, scale=1.0):
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    check(_hip.lib().nabu_sum_f32(x.numel(), ptr(x), scale, ptr(out), stream()), 'nabu_sum_f32')
    return out


def axpy_(y, x, a=1.0):
    check(_hip.lib().nabu_axpy_f32(x.numel(), a, ptr(x), ptr(y), stream()), 'nabu_axpy_f32')
    return y


def xent_loss_grad(logits, targets_dev, logit_len_dev, target_len_dev, grad_scale):
    """Returns (loss [B], dlogits [B,L,C])."""
    B, L, C = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    check(_hip.lib().nabu_xent_loss_grad(B, L, C, targets_dev.shape[1], ptr(_f32(logits, 'logits')),
                                         ptr(targets_dev), ptr(logit_len_dev), ptr(target_len_dev),
                                         grad_scale, ptr(loss), ptr(dlogits), stream()),
          'nabu_xent_loss_grad')
    return loss, dlogits


def xent_smooth_loss_grad(logits, targets_dev, logit_len_dev, target_len_dev, grad_scale, smoothing):
    """xent_loss_grad against the smoothed targets (1 - smoothing) * onehot + smoothing / C
    (nabu_xent_smooth_loss_grad): (loss [B], dlogits [B,L,C])"""
    B, L, C = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    check(_hip.lib().nabu_xent_smooth_loss_grad(B, L, C, targets_dev.shape[1], ptr(_f32(logits, 'logits')),
                                                ptr(targets_dev), ptr(logit_len_dev), ptr(target_len_dev),
                                                grad_scale, smoothing, ptr(loss), ptr(dlogits), stream()),
          'nabu_xent_smooth_loss_grad')
    return loss, dlogits


class RecurrentProfiler(object):
    """Times the recurrent kernel(s) of every BLSTM call with HIP events recorded by
    the library on the launch stream (nabu_blstm_set_profile_events).  Used by
    bench.py for the live roofline figure; off by default."""

    def __init__(self):
        self.hip = ctypes.CDLL('libamdhip64.so')
        self.records = []          # (kind, B, T_steps, H, ev_begin, ev_end)
        self.enabled = False

    def _event(self):
        ev = ctypes.c_void_p()
        err = self.hip.hipEventCreate(ctypes.byref(ev))
        if err:
            raise _hip.NabuHipError('hipEventCreate failed: %d' % err)
        return ev

    def arm(self, kind, plan):
        if not self.enabled:
            return
        b, e = self._event(), self._event()
        _hip.lib().nabu_blstm_set_profile_events(b, e)
        d = plan.desc
        self.records.append((kind, d.B, d.max_len if d.max_len > 0 else d.T, d.H, b, e))

    def disarm(self):
        if self.enabled:
            _hip.lib().nabu_blstm_set_profile_events(None, None)

    def collect(self):
        """[(kind, B, steps, H, milliseconds)] — call after a device synchronize."""
        out = []
        for kind, B, steps, H, b, e in self.records:
            ms = ctypes.c_float()
            err = self.hip.hipEventElapsedTime(ctypes.byref(ms), b, e)
            if err:
                raise _hip.NabuHipError('hipEventElapsedTime failed: %d' % err)
            out.append((kind, B, steps, H, ms.value))
            self.hip.hipEventDestroy(b)
            self.hip.hipEventDestroy(e)
        self.records = []
        return out


PROFILER = None


def enable_profiler():
    global PROFILER
    if PROFILER is None:
        PROFILER = RecurrentProfiler()
    PROFILER.enabled = True
    return PROFILER


_phase_hook = [None]       # keeps the ctypes trampoline alive


def set_phase_hook(fn):
    """fn() is called by nabu_blstm_bwd between its recurrent kernel(s) and its dense products
    (include/nabu_hip.h nabu_blstm_set_phase_hook); None switches the hook off"""
    if fn is None:
        _phase_hook[0] = None
        check(_hip.lib().nabu_blstm_set_phase_hook(None, None), 'nabu_blstm_set_phase_hook')
        return
    def trampoline(user):
        # ctypes prints and swallows an exception raised inside a C callback: keep it and let the
        # caller re-raise it once the C call has returned (take_phase_hook_error)
        try:
            fn()
        except BaseException as exc:                     # noqa: B902 — re-raised by the caller
            if _phase_hook_error[0] is None:
                _phase_hook_error[0] = exc
    _phase_hook[0] = _hip.PHASE_HOOK_T(trampoline)
    check(_hip.lib().nabu_blstm_set_phase_hook(ctypes.cast(_phase_hook[0], ctypes.c_void_p), None),
          'nabu_blstm_set_phase_hook')


_phase_hook_error = [None]


def take_phase_hook_error():
    """the first exception a phase hook raised since the last call (None if none); clears it"""
    exc, _phase_hook_error[0] = _phase_hook_error[0], None
    return exc


# called right before a recurrent launch is enqueued (forward and backward): the data-parallel
# trainer joins its communication stream here (the persistent kernels must run alone)
BEFORE_RECURRENT = [None]


def set_persist_timeout_ms(ms):
    """bound of the in-kernel waits of the persistent recurrent kernels (0 = the 200 ms default)"""
    check(_hip.lib().nabu_persist_set_timeout_us(int(ms * 1000)), 'nabu_persist_set_timeout_us')


def persist_workspaces():
    """[(tag, buffer)] of the workspaces whose first int32 is a persistent kernel's status word"""
    # 'speller': the persistent decoder kernel (speller_persist.hip)
    return [(tag, buf) for (dev, tag), buf in list(Workspace._bufs.items()) if tag in ('blstm', 'speller')]


def persist_status_error(tag, code):
    """the exception a non-zero status word of the `tag` workspace stands for"""
    return _hip.NabuHipError(
        'persistent %s kernel timed out waiting for a peer workgroup (code %d: block %d, %s); '
        'results of this step are invalid' % ('LSTM' if tag == 'blstm' else 'decoder', code, code // 4,
                                              {1: 'forward pass', 2: 'backward pass',
                                               3: 'start-up handshake'}.get(code % 4, '?')))


def check_persist_status(device=None):
    """Raise if a persistent recurrent kernel gave up (bounded-spin timeout); the
    status word is the first int32 of the 'blstm' / 'speller' workspace.  Synchronises."""
    for tag, buf in persist_workspaces():
        code = int(buf[:4].view(torch.int32).item())
        if code:
            buf[:4].zero_()
            raise persist_status_error(tag, code)


# ---------------------------------------------------------------- speller step kernels
def lstm_cell_fwd(step, seq_len_dev, z, bias, emb_rows, ids, c_prev, h_prev, acts, c_new, h_new):
    B, U = c_prev.shape
    check(_hip.lib().nabu_lstm_cell_fwd(B, U, step, ptr(seq_len_dev), ptr(z), ptr(bias), ptr(emb_rows),
                                        ptr(ids), ptr(c_prev), ptr(h_prev), ptr(acts), ptr(c_new), ptr(h_new),
                                        stream()), 'nabu_lstm_cell_fwd')


def lstm_cell_bwd(step, seq_len_dev, acts, c_new, c_prev, dh, dh2, dc_in, dz, dc_out):
    B, U = c_prev.shape
    check(_hip.lib().nabu_lstm_cell_bwd(B, U, step, ptr(seq_len_dev), ptr(acts), ptr(c_new), ptr(c_prev),
                                        ptr(dh), ptr(dh2), ptr(dc_in), ptr(dz), ptr(dc_out), stream()),
          'nabu_lstm_cell_bwd')


PROB_FNS = {'softmax': 0, 'sigmoid': 1, 'normalized_sigmoid': 2}


def attn_desc(B, Te, E, U, kind, K=0, F=0, prob_fn=0):
    return _hip.AttnDesc(ctypes.sizeof(_hip.AttnDesc), B, Te, E, U, kind, K, F, prob_fn)


def attn_fwd(desc, step, dec_len, enc_len, keys, values, q, v, conv_kernel, conv_proj, align_prev,
             ctx_prev, align, ctx, znorm=None):
    L = _hip.lib()
    nbytes = L.nabu_attn_fwd_ws_bytes(ctypes.byref(desc))
    ws = Workspace.get(nbytes, keys.device, 'attn_fwd') if nbytes else None
    check(L.nabu_attn_fwd(ctypes.byref(desc), step, ptr(dec_len), ptr(enc_len), ptr(keys), ptr(values),
                          ptr(q), ptr(v), ptr(conv_kernel), ptr(conv_proj), ptr(align_prev),
                          ptr(ctx_prev), ptr(align), ptr(ctx), ptr(znorm), ptr(ws), nbytes, stream()), 'nabu_attn_fwd')


def attn_bwd(desc, step, dec_len, enc_len, keys, values, q, v, conv_kernel, conv_proj, align_prev, align, ctx,
             dctx, dalign_in, dq, dkeys, dv_part, dcp_part, dck_part, dalign_out, znorm=None):
    """dv_part / dcp_part have B * attn_bwd_slices(desc) rows; ctx = this step's context"""
    L = _hip.lib()
    nbytes = L.nabu_attn_bwd_ws_bytes(ctypes.byref(desc))
    ws = Workspace.get(nbytes, keys.device, 'attn_bwd')
    check(L.nabu_attn_bwd(ctypes.byref(desc), step, ptr(dec_len), ptr(enc_len), ptr(keys), ptr(values),
                          ptr(q), ptr(v), ptr(conv_kernel), ptr(conv_proj), ptr(align_prev),
                          ptr(align), ptr(ctx), ptr(dctx), ptr(dalign_in), ptr(dq), ptr(dkeys), ptr(dv_part),
                          ptr(dcp_part), ptr(dck_part), ptr(dalign_out), ptr(znorm), ptr(ws), nbytes, stream()),
          'nabu_attn_bwd')


def attn_bwd_slices(desc):
    return _hip.lib().nabu_attn_bwd_slices(ctypes.byref(desc))


def mask_time_(x, len_dev):
    B, L, F = x.shape
    check(_hip.lib().nabu_mask_time_f32(B, L, F, ptr(x), ptr(len_dev), stream()), 'nabu_mask_time_f32')
    return x


def swap01(x):
    """[L,B,F] -> [B,L,F] (new tensor)."""
    L, B, F = x.shape
    y = torch.empty((B, L, F), dtype=x.dtype, device=x.device)
    check(_hip.lib().nabu_swap01_f32(L, B, F, ptr(x), ptr(y), stream()), 'nabu_swap01_f32')
    return y


def scatter_rows(ids, dz, dK):
    """dK[c,:] = sum_{i: ids[i]==c} dz[i,:]; ids [N] int32, dz [N,W], dK [C,W]."""
    N, W = dz.shape
    check(_hip.lib().nabu_scatter_rows_f32(dK.shape[0], N, W, ptr(ids), ptr(dz), ptr(dK), stream()),
          'nabu_scatter_rows_f32')
    return dK


def relu(x):
    y = torch.empty_like(x)
    check(_hip.lib().nabu_relu_f32(x.numel(), ptr(x), ptr(y), stream()), 'nabu_relu_f32')
    return y


def relu_bwd(y, dy):
    dx = torch.empty_like(y)
    check(_hip.lib().nabu_relu_bwd_f32(y.numel(), ptr(y), ptr(dy), ptr(dx), stream()), 'nabu_relu_bwd_f32')
    return dx


def layer_norm_fwd(x, gamma, beta, eps=1e-12):
    """x [B,...,F]: moments over everything but the batch axis (tf.contrib.layers.layer_norm)"""
    B, F = x.shape[0], x.shape[-1]
    N = x.numel() // B
    y = torch.empty_like(x)
    mean = torch.empty(B, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, dtype=torch.float32, device=x.device)
    check(_hip.lib().nabu_layer_norm_fwd(B, N, F, ptr(x), ptr(gamma), ptr(beta), eps, ptr(y), ptr(mean), ptr(rstd),
                                         stream()), 'nabu_layer_norm_fwd')
    return y, mean, rstd


def layer_norm_bwd(x, gamma, dy, mean, rstd):
    B, F = x.shape[0], x.shape[-1]
    N = x.numel() // B
    dx = torch.empty_like(x)
    dgp = torch.empty((B, F), dtype=torch.float32, device=x.device)
    dbp = torch.empty((B, F), dtype=torch.float32, device=x.device)
    check(_hip.lib().nabu_layer_norm_bwd(B, N, F, ptr(x), ptr(gamma), ptr(dy), ptr(mean), ptr(rstd), ptr(dx),
                                         ptr(dgp), ptr(dbp), stream()), 'nabu_layer_norm_bwd')
    return dx, dgp, dbp


def splice_stack(x, len_dev, context, N, ld):
    """[N, ld] = the spliced frames (0, +1, -1, ..., +-(context-1)) of x [B,T,F] stacked batch-major, zero columns
    from (2 context - 1) F on (nabu_splice_stack_f32); N = sum of the lengths (the caller's host copy)"""
    B, T, F = x.shape
    out = torch.empty((N, ld), dtype=torch.float32, device=x.device)
    if N:
        check(_hip.lib().nabu_splice_stack_f32(B, T, F, int(context), ptr(_f32(x, 'x')), ptr(len_dev), ptr(out), ld,
                                               stream()), 'nabu_splice_stack_f32')
    return out


def unstack_rows(rows, len_dev, B, Tm):
    """rows [N,H] -> [B,Tm,H], zero past each length (nabu_unstack_rows_f32)"""
    H = rows.shape[1]
    out = torch.empty((B, Tm, H), dtype=torch.float32, device=rows.device)
    check(_hip.lib().nabu_unstack_rows_f32(B, Tm, H, ptr(len_dev), ptr(_f32(rows, 'rows')), ptr(out), stream()),
          'nabu_unstack_rows_f32')
    return out


def stack_rows(g, len_dev, N):
    """g [B,Tm,H] -> rows [N,H] of the valid frames (nabu_stack_rows_f32, the adjoint of unstack_rows)"""
    B, Tm, H = g.shape
    rows = torch.empty((N, H), dtype=torch.float32, device=g.device)
    if N:
        check(_hip.lib().nabu_stack_rows_f32(B, Tm, H, ptr(len_dev), ptr(_f32(g, 'g')), ptr(rows), stream()),
              'nabu_stack_rows_f32')
    return rows


def rows_relu_ln_fwd(z, gamma, beta, eps=1e-12):
    """(y, mean, rstd) of relu then per-row layer norm of z [N,F] (nabu_rows_relu_ln_fwd), or None when the kernel
    does not take F (NABU_EUNSUP: the caller composes relu + layer_norm_fwd)"""
    N, F = z.shape
    y = torch.empty_like(z)
    mean = torch.empty(N, dtype=torch.float32, device=z.device)
    rstd = torch.empty(N, dtype=torch.float32, device=z.device)
    code = _hip.lib().nabu_rows_relu_ln_fwd(N, F, ptr(_f32(z, 'z')), ptr(gamma), ptr(beta), eps, ptr(y), ptr(mean),
                                            ptr(rstd), stream())
    if code == NABU_EUNSUP:
        return None
    check(code, 'nabu_rows_relu_ln_fwd')
    return y, mean, rstd


def rows_relu_ln_bwd(z, dy, gamma, mean, rstd):
    """(dz, dgamma_part [P,F], dbeta_part [P,F]) of rows_relu_ln_fwd (reduce the partials with colsum)"""
    N, F = z.shape
    L = _hip.lib()
    P = L.nabu_rows_relu_ln_bwd_parts(N)
    dz = torch.empty_like(z)
    dgp = torch.empty((P, F), dtype=torch.float32, device=z.device)
    dbp = torch.empty((P, F), dtype=torch.float32, device=z.device)
    check(L.nabu_rows_relu_ln_bwd(N, F, ptr(z), ptr(_f32(dy, 'dy')), ptr(gamma), ptr(mean), ptr(rstd), ptr(dz),
                                  ptr(dgp), ptr(dbp), stream()), 'nabu_rows_relu_ln_bwd')
    return dz, dgp, dbp


def xent_wide_loss_grad(logits, targets_dev, logit_len_dev, target_len_dev, grad_scale):
    """xent_loss_grad's contract on the wide-class kernel (nabu_xent_wide_loss_grad): (loss [B], dlogits [B,L,C])"""
    B, L, C = logits.shape
    lib = _hip.lib()
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws_bytes = lib.nabu_xent_wide_ws_bytes(B, L)
    ws = Workspace.get(ws_bytes, logits.device, 'xent_wide')
    check(lib.nabu_xent_wide_loss_grad(B, L, C, targets_dev.shape[1], ptr(_f32(logits, 'logits')), ptr(targets_dev),
                                       ptr(logit_len_dev), ptr(target_len_dev), grad_scale, ptr(loss), ptr(dlogits),
                                       ptr(ws), ws_bytes, stream()), 'nabu_xent_wide_loss_grad')
    return loss, dlogits


def xent_wide_smooth_loss_grad(logits, targets_dev, logit_len_dev, target_len_dev, grad_scale, smoothing):
    """xent_smooth_loss_grad's contract on the wide-class kernel (nabu_xent_wide_smooth_loss_grad)"""
    B, L, C = logits.shape
    lib = _hip.lib()
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    ws_bytes = lib.nabu_xent_wide_ws_bytes(B, L)
    ws = Workspace.get(ws_bytes, logits.device, 'xent_wide')
    check(lib.nabu_xent_wide_smooth_loss_grad(B, L, C, targets_dev.shape[1], ptr(_f32(logits, 'logits')),
                                              ptr(targets_dev), ptr(logit_len_dev), ptr(target_len_dev), grad_scale,
                                              smoothing, ptr(loss), ptr(dlogits), ptr(ws), ws_bytes, stream()),
          'nabu_xent_wide_smooth_loss_grad')
    return loss, dlogits


def log_softmax_prior(x, len_dev, logprior):
    """x - logsumexp(x) - logprior over the last axis of x [B,T,C] for t < len[b], 0 elsewhere"""
    B, T, C = x.shape
    out = torch.empty_like(x)
    check(_hip.lib().nabu_log_softmax_prior_f32(B, T, C, ptr(_f32(x, 'x')), ptr(len_dev), ptr(logprior), ptr(out),
                                                stream()), 'nabu_log_softmax_prior_f32')
    return out


def ceil_div_i32(x, d):
    out = torch.empty_like(x)
    check(_hip.lib().nabu_ceil_div_i32(x.numel(), ptr(x), int(d), ptr(out), stream()), 'nabu_ceil_div_i32')
    return out


def batch_unpack(segs, packed, packed_bytes=None):
    """One launch writes every padded tensor of a packed batch (processing/prefetch.py lays the buffer out).
    segs: up to 8 (rows, width, max_len, len_off, row_off, data_off, out, out_len) with out a contiguous
    [rows, max_len * width] (any shape of that size) float32 or int32 device tensor and out_len a [rows] int32 one;
    packed: the uint8 device buffer the batch was uploaded into."""
    if packed_bytes is None:
        packed_bytes = packed.numel() * packed.element_size()
    arr = (_hip.BatchSeg * len(segs))()
    for d, (rows, width, max_len, len_off, row_off, data_off, out, out_len) in zip(arr, segs):
        if out.element_size() != 4 or out.numel() != rows * max_len * width:
            raise _hip.NabuHipError('batch_unpack: out must hold rows * max_len * width 4-byte elements')
        if out_len.dtype != torch.int32 or out_len.numel() != rows:
            raise _hip.NabuHipError('batch_unpack: out_len must be [rows] int32')
        d.rows, d.width, d.max_len, d.reserved = int(rows), int(width), int(max_len), 0
        d.len_off, d.row_off, d.data_off = int(len_off), int(row_off), int(data_off)
        d.out, d.out_len = ptr(out), ptr(out_len)
    check(_hip.lib().nabu_batch_unpack(len(segs), ctypes.cast(arr, ctypes.c_void_p), ptr(packed), int(packed_bytes),
                                       stream()), 'nabu_batch_unpack')


# --------------------------------------------------------------------------
# inference decoders (decode.hip)
def ctc_beam_search(logits, logit_len, beam_width=100, merge_repeated=True):
    """tf.nn.ctc_beam_search_decoder(top_paths=1) on batch-major logits [B,T,C]:
    returns (ids [B,T] int32 padded with -1, lengths [B] int32, log-probabilities [B])"""
    B, T, C = logits.shape
    logits = logits.contiguous()
    lib = _hip.lib()
    nbytes = lib.nabu_ctc_beam_ws_bytes(B, T, C, int(beam_width))
    ws = _hip.Workspace.get(nbytes, logits.device, 'ctc_beam')
    ids = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    lens = torch.empty((B,), dtype=torch.int32, device=logits.device)
    lp = torch.empty((B,), dtype=torch.float32, device=logits.device)
    check(lib.nabu_ctc_beam_search(B, T, C, int(beam_width), int(bool(merge_repeated)), ptr(logits),
                                   ptr(logit_len), ptr(ids), ptr(lens), ptr(lp), ptr(ws), nbytes, stream()),
          'nabu_ctc_beam_search')
    return ids, lens, lp


def _lm_table(table, C, lm_order):
    """the device table [C^(order-1), C] of a label n-gram (processing/ngram_lm.py), checked"""
    table = _f32(table, 'lm_table')
    lm_order = int(lm_order)
    if lm_order < 1:
        raise _hip.NabuHipError('lm_order must be at least 1, got %d' % lm_order)
    if C ** lm_order > _hip.LM_MAX_ENTRIES:
        raise _hip.NabuHipError('an n-gram table of %d^%d entries exceeds the limit of 2^24 entries (64 MiB)' % (C, lm_order))
    if tuple(table.shape) != (C ** (lm_order - 1), C):
        raise _hip.NabuHipError('lm_table has shape %r, order %d over %d symbols needs %r'
                                % (tuple(table.shape), lm_order, C, (C ** (lm_order - 1), C)))
    return table.contiguous()


def ctc_beam_search_lm(logits, logit_len, lm_table, lm_order, lm_weight, insertion_bonus=0.0, beam_width=100,
                       merge_repeated=True):
    """ctc_beam_search with a label n-gram (nabu_ctc_beam_search_lm: the scorer hooks of TF's CTC beam search).
    lm_table [C^(lm_order-1), C] float32 log-probabilities on the device, symbol C-1 the boundary; appending a label
    adds lm_weight * lm_table[ctx, label] + insertion_bonus, the end adds lm_weight * lm_table[ctx, C-1].
    Returns (ids, lengths, log-probabilities) as ctc_beam_search; the log-probabilities include the LM terms."""
    B, T, C = logits.shape
    logits = logits.contiguous()
    table = _lm_table(lm_table, C, lm_order)
    lib = _hip.lib()
    nbytes = lib.nabu_ctc_beam_lm_ws_bytes(B, T, C, int(beam_width))
    ws = _hip.Workspace.get(nbytes, logits.device, 'ctc_beam')
    ids = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    lens = torch.empty((B,), dtype=torch.int32, device=logits.device)
    lp = torch.empty((B,), dtype=torch.float32, device=logits.device)
    check(lib.nabu_ctc_beam_search_lm(B, T, C, int(beam_width), int(bool(merge_repeated)), ptr(logits), ptr(logit_len),
                                      ptr(table), int(lm_order), float(lm_weight), float(insertion_bonus), ptr(ids),
                                      ptr(lens), ptr(lp), ptr(ws), nbytes, stream()), 'nabu_ctc_beam_search_lm')
    return ids, lens, lp


def edit_distance(hyp, hyp_len, truth, truth_len):
    """Levenshtein distance per row: hyp [B,Lh], truth [B,Lt] int32 with their lengths -> [B] int32"""
    B = hyp.shape[0]
    hyp, truth = hyp.contiguous(), truth.contiguous()
    dist = torch.empty((B,), dtype=torch.int32, device=hyp.device)
    check(_hip.lib().nabu_edit_distance(B, ptr(hyp) if hyp.numel() else None, hyp.shape[1], ptr(hyp_len),
                                        ptr(truth) if truth.numel() else None, truth.shape[1],
                                        ptr(truth_len), ptr(dist), stream()), 'nabu_edit_distance')
    return dist


MWER_MAX_NBEST = 16


def mwer_prepare(sequences, lengths, scores, targets, target_len, C, ldt=None):
    """beams of the attention beam search -> stacked teacher-forcing targets (nabu_mwer_prepare), slot-major: row
    n * B + b is hypothesis n of utterance b, slot N the reference.  sequences [B,N,S] int32 (a view with a longer row
    stride is taken as it is), lengths [B,N], scores [B,N], targets [B,ldr] int32, target_len [B] (counts the end label).
    Returns (stk_targets [(N+1)*B, ldt], stk_len [(N+1)*B], hyp_len [N*B], valid [N*B]); ldt defaults to
    max(S + 1, ldr)."""
    B, N, S = sequences.shape
    if not sequences.is_cuda or sequences.dtype != torch.int32:
        raise _hip.NabuHipError('sequences must be an int32 tensor on the GPU, got %s on %s'
                                % (sequences.dtype, sequences.device))
    if S and sequences.stride(2) == 1 and sequences.stride(0) == N * sequences.stride(1) and sequences.stride(1) >= S:
        lds = sequences.stride(1)               # the beam search's [B,N,max_steps] buffer cut to the steps it took
    else:
        sequences, lds = sequences.contiguous(), S
    seq_ptr = sequences.data_ptr() if S else None
    targets = targets.contiguous()
    ldr = targets.shape[1]
    ldt = max(S + 1, ldr) if ldt is None else int(ldt)
    dev = sequences.device
    stk_targets = torch.empty(((N + 1) * B, ldt), dtype=torch.int32, device=dev)
    stk_len = torch.empty((N + 1) * B, dtype=torch.int32, device=dev)
    hyp_len = torch.empty(N * B, dtype=torch.int32, device=dev)
    valid = torch.empty(N * B, dtype=torch.int32, device=dev)
    check(_hip.lib().nabu_mwer_prepare(B, N, S, lds, int(C), seq_ptr, ptr(lengths.contiguous()),
                                       ptr(_f32(scores, 'scores').contiguous()), ldr, ptr(targets), ptr(target_len), ldt,
                                       ptr(stk_targets), ptr(stk_len), ptr(hyp_len), ptr(valid), stream()),
          'nabu_mwer_prepare')
    return stk_targets, stk_len, hyp_len, valid


def rows_tile(x, R):
    """y[r * B + b] = x[b] for r < R: x [B, ...] -> [R * B, ...] (nabu_rows_tile_f32)"""
    x = _f32(x, 'x').contiguous()
    B = x.shape[0]
    y = torch.empty((R * B,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    check(_hip.lib().nabu_rows_tile_f32(int(R), B, x.numel() // B, ptr(x), ptr(y), stream()), 'nabu_rows_tile_f32')
    return y


def rows_tile_bwd(dy, R):
    """dx[b] = sum_r dy[r * B + b] in the order r = 0..R-1: dy [R * B, ...] -> [B, ...] (nabu_rows_tile_bwd_f32)"""
    dy = _f32(dy, 'dy').contiguous()
    B = dy.shape[0] // R
    if B * R != dy.shape[0]:
        raise ValueError('rows_tile_bwd: %d rows are no multiple of R = %d' % (dy.shape[0], R))
    dx = torch.empty((B,) + tuple(dy.shape[1:]), dtype=torch.float32, device=dy.device)
    check(_hip.lib().nabu_rows_tile_bwd_f32(int(R), B, dx.numel() // B, ptr(dy), ptr(dx), stream()),
          'nabu_rows_tile_bwd_f32')
    return dx


def mwer_loss_grad(logits, stk_targets, stk_len, errors, valid, ce_weight, grad_scale):
    """the MWER objective and its gradient in one launch (nabu_mwer_loss_grad): logits [(N+1)*B, L, C] of the stacked
    targets of mwer_prepare, errors / valid [N*B] int32.  Returns (loss [B], risk [B], nll_ref [B], dlogits)."""
    rows, L, C = logits.shape
    NB = valid.numel()
    B = rows - NB
    if B <= 0 or NB % B:
        raise ValueError('mwer_loss_grad: %d logit rows and %d hypotheses do not stack' % (rows, NB))
    dev = logits.device
    loss, risk, nll_ref = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
    dlogits = torch.empty_like(logits)
    check(_hip.lib().nabu_mwer_loss_grad(B, NB // B, L, C, stk_targets.shape[1], ptr(_f32(logits, 'logits')),
                                         ptr(stk_targets), ptr(stk_len), ptr(errors), ptr(valid), float(ce_weight),
                                         float(grad_scale), ptr(loss), ptr(risk), ptr(nll_ref), ptr(dlogits), stream()),
          'nabu_mwer_loss_grad')
    return loss, risk, nll_ref, dlogits


def beam_prune(logits, logprobs, lengths, finished, seen, temperature=1.0, length_penalty=0.0):
    """one expand+prune step of the attention beam search; logits [B,W,C]; the [B,W] state tensors
    are updated in place.  Returns (pred_ids, parent, stay, all_seen)"""
    B, W, C = logits.shape
    dev = logits.device
    pred = torch.empty((B, W), dtype=torch.int32, device=dev)
    parent, stay = torch.empty_like(pred), torch.empty_like(pred)
    all_seen = torch.empty((B,), dtype=torch.int32, device=dev)
    scratch = torch.empty((B, W * C + W), dtype=torch.float32, device=dev)
    check(_hip.lib().nabu_beam_prune(B, W, C, ptr(logits.contiguous()), float(temperature), float(length_penalty),
                                     ptr(logprobs), ptr(lengths), ptr(finished), ptr(seen), ptr(pred),
                                     ptr(parent), ptr(stay), ptr(all_seen), ptr(scratch), stream()),
          'nabu_beam_prune')
    return pred, parent, stay, all_seen


def beam_prune_joint(logits, delta, ctc_weight, logprobs, lengths, finished, seen, temperature=1.0, length_penalty=0.0):
    """beam_prune with the CTC term: delta [B,W,C] from ctc_prefix_score, weighted by ctc_weight in [0, 1)"""
    B, W, C = logits.shape
    dev = logits.device
    pred = torch.empty((B, W), dtype=torch.int32, device=dev)
    parent, stay = torch.empty_like(pred), torch.empty_like(pred)
    all_seen = torch.empty((B,), dtype=torch.int32, device=dev)
    scratch = torch.empty((B, W * C + W), dtype=torch.float32, device=dev)
    check(_hip.lib().nabu_beam_prune_joint(B, W, C, ptr(logits.contiguous()), ptr(_f32(delta, 'delta').contiguous()),
                                           float(ctc_weight), float(temperature), float(length_penalty), ptr(logprobs),
                                           ptr(lengths), ptr(finished), ptr(seen), ptr(pred), ptr(parent), ptr(stay),
                                           ptr(all_seen), ptr(scratch), stream()), 'nabu_beam_prune_joint')
    return pred, parent, stay, all_seen


def beam_prune_lm(logits, delta, ctc_weight, lm_table, lm_order, lm_weight, ctx, logprobs, lengths, finished, seen,
                  temperature=1.0, length_penalty=0.0):
    """beam_prune with the label n-gram term lm_weight * lm_table[ctx[w], c] on every live beam's candidates, and with
    the CTC term of beam_prune_joint where delta is not None.  ctx [B,W] int32: the beams' contexts (not changed).
    Returns (pred_ids, parent, stay, all_seen, the survivors' contexts [B,W] int32)"""
    B, W, C = logits.shape
    dev = logits.device
    table = _lm_table(lm_table, C, lm_order)
    pred = torch.empty((B, W), dtype=torch.int32, device=dev)
    parent, stay, ctx_out = torch.empty_like(pred), torch.empty_like(pred), torch.empty_like(pred)
    all_seen = torch.empty((B,), dtype=torch.int32, device=dev)
    scratch = torch.empty((B, W * C + W), dtype=torch.float32, device=dev)
    if ctx.dtype != torch.int32 or tuple(ctx.shape) != (B, W):
        raise _hip.NabuHipError('ctx must be int32 [B,W], got %s %r' % (ctx.dtype, tuple(ctx.shape)))
    check(_hip.lib().nabu_beam_prune_lm(B, W, C, ptr(logits.contiguous()),
                                        None if delta is None else ptr(_f32(delta, 'delta').contiguous()),
                                        float(ctc_weight), ptr(table), int(lm_order), float(lm_weight),
                                        ptr(ctx.contiguous()), ptr(ctx_out), float(temperature), float(length_penalty),
                                        ptr(logprobs), ptr(lengths), ptr(finished), ptr(seen), ptr(pred), ptr(parent),
                                        ptr(stay), ptr(all_seen), ptr(scratch), stream()), 'nabu_beam_prune_lm')
    return pred, parent, stay, all_seen, ctx_out


class CtcPrefixState(object):
    """The CTC prefix-scoring state of a beam (ctc_prefix.hip): state [B,W,T,2] = (r_n, r_b) per frame, psi [B,W],
    last [B,W] (-1: the empty hypothesis), with the logits [B,T,C], their lengths and the per-frame normalisers
    norm [B,T,2] they belong to"""

    def __init__(self, logits, enc_len, norm, W, state=None, psi=None, last=None):
        B, T, _ = logits.shape
        dev = logits.device
        self.logits, self.enc_len, self.norm, self.W = logits, enc_len, norm, int(W)
        self.state = torch.empty((B, W, T, 2), dtype=torch.float32, device=dev) if state is None else state
        self.psi = torch.empty((B, W), dtype=torch.float32, device=dev) if psi is None else psi
        self.last = torch.empty((B, W), dtype=torch.int32, device=dev) if last is None else last

    def _dims(self):
        B, T, C = self.logits.shape
        return B, self.W, T, C


def ctc_prefix_prepare(logits, enc_len, beam_width):
    """once per search: the normalisers of logits [B,T,C] and the state of the empty hypothesis in all beam slots"""
    logits = _f32(logits, 'logits').contiguous()
    B, T, _ = logits.shape
    norm = torch.empty((B, T, 2), dtype=torch.float32, device=logits.device)
    s = CtcPrefixState(logits, enc_len, norm, beam_width)
    check(_hip.lib().nabu_ctc_prefix_prepare(*s._dims(), ptr(logits), ptr(enc_len), ptr(norm), ptr(s.state), ptr(s.psi),
                                             ptr(s.last), stream()), 'nabu_ctc_prefix_prepare')
    return s


def ctc_prefix_score(s, finished):
    """delta [B,W,C] = psi(g.c) - psi(g) of every hypothesis of the beam and every class (C-1: the end label)"""
    B, W, T, C = s._dims()
    delta = torch.empty((B, W, C), dtype=torch.float32, device=s.logits.device)
    check(_hip.lib().nabu_ctc_prefix_score(B, W, T, C, ptr(s.logits), ptr(s.enc_len), ptr(s.norm), ptr(s.state), ptr(s.psi),
                                           ptr(s.last), ptr(finished), ptr(delta), stream()), 'nabu_ctc_prefix_score')
    return delta


def ctc_prefix_advance(s, parent, stay, pred):
    """the state of the survivors of a pruning step (parent, stay, pred [B,W] as beam_prune returns them): a new
    CtcPrefixState, `s` is left as it was"""
    n = CtcPrefixState(s.logits, s.enc_len, s.norm, s.W)
    check(_hip.lib().nabu_ctc_prefix_advance(*s._dims(), ptr(s.logits), ptr(s.enc_len), ptr(s.norm), ptr(s.state),
                                             ptr(s.psi), ptr(s.last), ptr(parent), ptr(stay), ptr(pred), ptr(n.state),
                                             ptr(n.psi), ptr(n.last), stream()), 'nabu_ctc_prefix_advance')
    return n


def beam_gather(fresh, old, parent, stay):
    B, W, F = fresh.shape
    dst = torch.empty_like(fresh)
    check(_hip.lib().nabu_beam_gather(B, W, F, ptr(fresh.contiguous()), ptr(old.contiguous()), ptr(parent),
                                      ptr(stay), ptr(dst), stream()), 'nabu_beam_gather')
    return dst


def sample_advance(logits, seed, offset, t, sequences, lengths, finished, nll):
    """one step of the sampled decode on its own; logits [B,C]; sequences [B,max_steps], lengths, finished and
    nll [B] are updated in place.  Returns (next_ids [B], all_finished [1])"""
    B, C = logits.shape
    next_ids = torch.empty((B,), dtype=torch.int32, device=logits.device)
    all_finished = torch.empty((1,), dtype=torch.int32, device=logits.device)
    check(_hip.lib().nabu_sample_advance(B, C, ptr(logits.contiguous()), seed, offset, int(t), sequences.shape[1],
                                         ptr(sequences), ptr(lengths), ptr(finished), ptr(nll), ptr(next_ids),
                                         ptr(all_finished), stream()), 'nabu_sample_advance')
    return next_ids, all_finished


def persist_clocks(device=None):
    """{'fwd': GHz, 'bwd': GHz} — the shader clock the chip sustained under the LAST fp16-plane recurrent launch of each
    pass on this device's 'blstm' workspace (lstm_persist_dev.h, clock_stamp: shader-cycle and 100 MHz wall-clock ticks
    left by block 0 at the start and the end of the launch).  None for a pass that has not run.  Synchronises."""
    out = {'fwd': None, 'bwd': None}
    for (dev, tag), buf in list(Workspace._bufs.items()):
        if tag != 'blstm' or (device is not None and dev != str(device)):
            continue
        w = buf[4 * 280:4 * 288].view(torch.int32).cpu().tolist()
        for i, name in enumerate(('fwd', 'bwd')):
            c0, w0, c1, w1 = w[4 * i:4 * i + 4]
            dc, dw = (c1 - c0) & 0xFFFFFFFF, (w1 - w0) & 0xFFFFFFFF
            if dw > 0 and dc > 0:
                out[name] = round(dc / dw * 0.1, 4)
    return out
