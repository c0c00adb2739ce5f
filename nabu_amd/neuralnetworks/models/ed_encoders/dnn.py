"""DNN encoder of the Kaldi-hybrid recipe (reference: nabu/neuralnetworks/models/ed_encoders/dnn.py:11-66).

Per input: splice the frames with `context` (dnn.py:33-44), stack the valid frames batch-major (ops.stack_seq),
`num_layers` x [fully_connected (linear + ReLU), layer_norm if layer_norm == 'True', dropout if dropout < 1 and
training], unstack to [B, max(len), H] (ops.unstack_seq).  The lengths are returned unchanged.

* Splice order is the reference's: blocks of F columns for shifts 0, +1, -1, +2, -2, ..., +(c-1), -(c-1); "+i"
  reads frame t+i of the PADDED batch tensor (zero past its T, and whatever the padding holds past the utterance's
  length — the pipelines of this project zero it).  The splice and the stacking are one kernel
  (nabu_splice_stack_f32).
* The spliced matrix has ld = (2c-1)F rounded up to a multiple of 32 columns (zeros past (2c-1)F) and the first
  layer's weights are multiplied through a zero-padded copy, so the first product's reduction length is a multiple
  of 32 and the bf16 kernels take it at the requested `gemm_precision`; with an unpadded K they run exact fp32.
  Products whose other dimensions the bf16 kernels do not take (a frame count N % 4 != 0, the weight gradients'
  reduction over N frames) run exact fp32 — never a lower precision than asked (include/nabu_hip.h, nabu_gemm_ex).
* layer_norm on the 2-D stacked rows takes its moments PER FRAME over F (variables LayerNorm[_k]/{beta,gamma},
  variance_epsilon 1e-12); ReLU and layer norm are one kernel each way (nabu_rows_relu_ln_fwd/_bwd), or the relu and
  layer_norm kernels of the DNN decoder with B = N rows where the fused kernel does not take F.
* Dropout (keep probability `dropout`) is components/ops.seq_dropout over the stacked [N, H] rows.
* input_noise: the key is read (defaults/dnn.cfg) and IGNORED, as the reference's dnn.py never applies it.
* The input features never need a gradient: the first layer has no input-gradient product, and a taped input
  raises instead of receiving a wrong gradient.

Variables: DNN/<input>/layer<i>/{weights,biases}, DNN/<input>/LayerNorm[_<i>]/{beta,gamma}."""
import torch

from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, requires_grad, SeqLen
from nabu_amd.neuralnetworks.components import ops
from nabu_amd.neuralnetworks.models.ed_decoders import dnn_decoder
from nabu_amd.neuralnetworks.models.ed_encoders import ed_encoder
from nabu_amd.neuralnetworks.models.ed_encoders.listener import SPEC_AUGMENT_KEYS

SPLICE_LD_MULTIPLE = 32     # the bf16 product kernels' reduction tile


def _linear(x, K, ld, num_outputs, scope, precision, first):
    """fully_connected's linear part on stacked rows x [N, ld] whose first K columns are the input: weights [K, H]
    xavier, biases zeros.  Returns z [N, H]."""
    N = x.shape[0]
    with vs.variable_scope(scope):
        W = vs.get_variable('weights', [K, num_outputs])
        b = vs.get_variable('biases', [num_outputs], vs.zeros)
    if ld != K:
        Wm = torch.zeros((ld, num_outputs), dtype=torch.float32, device=x.device)
        Wm[:K].copy_(W.data)
    else:
        Wm = W.data
    z = torch.empty((N, num_outputs), dtype=torch.float32, device=x.device)
    hip.gemm(x, Wm, z, bias=b.data, precision=precision)

    def backward(dz):
        dz = dz.contiguous()
        for v in (W, b):
            if v.grad is None:
                v.grad = torch.zeros_like(v.data)
        # dW = x[:, :K]^T dz, db = colsum(dz) (each variable is read once per step: the gradients are overwritten)
        hip.gemm(x, dz, W.grad, trans_a=True, M=K, N=num_outputs, K=N, lda=ld, ldb=num_outputs,
                 ldc=num_outputs, precision=precision)
        hip.colsum(dz, b.grad)
        if first:
            return [None]
        dx = torch.empty_like(x)
        hip.gemm(dz, W.data, dx, trans_b=True, precision=precision)          # dx = dz W^T
        return [dx]
    record([x], [z], backward, params=(W, b))
    return z


def _relu_layer_norm(z, scope):
    """ReLU then tf.contrib.layers.layer_norm of the 2-D rows z [N, F] (moments per row)"""
    F = z.shape[1]
    with vs.variable_scope(scope):
        beta = vs.get_variable('beta', [F], vs.zeros)
        gamma = vs.get_variable('gamma', [F], dnn_decoder.ones)
    fwd = hip.rows_relu_ln_fwd(z, gamma.data, beta.data)
    if fwd is None:                                  # F the fused kernel does not take: same semantics, more launches
        r = hip.relu(z)
        y, mean, rstd = hip.layer_norm_fwd(r, gamma.data, beta.data)

        def backward(dy):
            dr, dgp, dbp = hip.layer_norm_bwd(r, gamma.data, dy.contiguous(), mean, rstd)
            _accumulate(gamma, beta, dgp, dbp)
            return [hip.relu_bwd(r, dr)]
    else:
        y, mean, rstd = fwd

        def backward(dy):
            dz, dgp, dbp = hip.rows_relu_ln_bwd(z, dy.contiguous(), gamma.data, mean, rstd)
            _accumulate(gamma, beta, dgp, dbp)
            return [dz]
    record([z], [y], backward, params=(beta, gamma))
    return y


def _accumulate(gamma, beta, dgp, dbp):
    for v in (beta, gamma):
        if v.grad is None:
            v.grad = torch.zeros_like(v.data)
    hip.colsum(dgp, gamma.grad)
    hip.colsum(dbp, beta.grad)


def splice_ld(width, context):
    """columns of the spliced matrix of `width`-wide frames: (2 context - 1) width rounded up to SPLICE_LD_MULTIPLE"""
    K = (2 * int(context) - 1) * int(width)
    return -(-K // SPLICE_LD_MULTIPLE) * SPLICE_LD_MULTIPLE


class DNN(ed_encoder.EDEncoder):
    """cfg keys: num_units, num_layers, input_noise (ignored, as in the reference), dropout (keep probability),
    context, layer_norm, gemm_precision (build addition).  The SpecAugment keys of the recurrent encoders are refused:
    the targets are frame-synchronous alignments, which a time warp would break."""

    def __init__(self, conf, constraint, name=None):
        super(DNN, self).__init__(conf, constraint, name)
        found = [k for k in SPEC_AUGMENT_KEYS if k in self.conf]
        if found:
            raise Exception('DNN encoder: the SpecAugment keys (%s) are not supported: the targets are alignments, one '
                            'per frame, and the augmentation moves and masks frames' % ', '.join(found))

    def encode(self, inputs, input_seq_length, is_training):
        precision = self.conf.get('gemm_precision', 'default')
        context, units = int(self.conf['context']), int(self.conf['num_units'])
        keep = float(self.conf['dropout'])
        encoded = {}
        for name, x in inputs.items():
            if requires_grad(x):
                raise Exception('DNN encoder: the input %s depends on a parameter; the first layer computes no input '
                                'gradient' % name)
            lens = SeqLen.wrap(input_seq_length[name], x.device)
            x = x if x.is_contiguous() else x.contiguous()
            B, T, F = x.shape
            N = int(lens.host.clip(0, T).sum())
            Tm = lens.max()
            K, ld = (2 * context - 1) * F, splice_ld(F, context)
            with vs.variable_scope(name):
                h = hip.splice_stack(x, lens.dev, context, N, ld)              # dnn.py:33-44 + ops.stack_seq
                width, hld = K, ld
                for i in range(int(self.conf['num_layers'])):                  # dnn.py:53-63
                    z = _linear(h, width, hld, units, 'layer%d' % i, precision, first=i == 0)
                    if self.conf['layer_norm'] == 'True':
                        h = _relu_layer_norm(z, 'LayerNorm' if i == 0 else 'LayerNorm_%d' % i)
                    else:
                        h = dnn_decoder.relu(z)
                    if keep < 1 and is_training:
                        h = ops.seq_dropout(h, keep, ops.global_rng())
                    width = hld = units
                out = hip.unstack_rows(h, lens.dev, B, Tm)                    # ops.unstack_seq

                def backward(dout, lens=lens, N=N):
                    return [hip.stack_rows(dout.contiguous(), lens.dev, N)]
                record([h], [out], backward)
                encoded[name] = out
        return encoded, dict(input_seq_length)
