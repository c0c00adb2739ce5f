"""Float64 reference of the DNN encoder + DNN decoder (num_layers = 0) + average_cross_entropy of the Kaldi-hybrid
recipe, written in torch autograd on the CPU from the reference's semantics (nabu/neuralnetworks/models/ed_encoders/
dnn.py, components/ops.py stack_seq / unstack_seq, tf.contrib.layers.layer_norm on 2-D rows), not from the kernels.
Dropout masks come from the host Philox (oracle/philox.py)."""
import numpy as np
import torch

from oracle import philox as P

EPS = 1e-12


def splice(x, context):
    """concat([x, x(+1), x(-1), x(+2), x(-2), ...], axis=2) over the padded batch tensor (dnn.py:33-44)"""
    T = x.shape[1]
    times = [x]
    for i in range(1, context):
        plus = torch.zeros_like(x)
        minus = torch.zeros_like(x)
        if i < T:
            plus[:, :T - i] = x[:, i:]
            minus[:, i:] = x[:, :T - i]
        times += [plus, minus]
    return torch.cat(times, 2)


def stack_seq(x, lens):
    return torch.cat([x[b, :int(n)] for b, n in enumerate(lens)], 0)


def unstack_seq(rows, lens):
    Tm = int(max(lens))
    out = rows.new_zeros((len(lens), Tm, rows.shape[1]))
    o = 0
    for b, n in enumerate(lens):
        out[b, :int(n)] = rows[o:o + int(n)]
        o += int(n)
    return out


def relu_layer_norm(z, gamma, beta):
    r = torch.relu(z)
    mu = r.mean(1, keepdim=True)
    var = ((r - mu) ** 2).mean(1, keepdim=True)
    return (r - mu) / torch.sqrt(var + EPS) * gamma + beta


def dropout_masks(N, H, num_layers, keep, seed, offset0):
    """the masks seq_dropout draws for layers 0..num_layers-1: stream (seed, offset0 + i + 1) over the [N, H] rows"""
    return [P.dropout_scale(N * H, keep, seed, offset0 + i + 1).astype(np.float64).reshape(N, H)
            for i in range(num_layers)]


def names(input_name, output_name, num_layers, layer_norm=True):
    out = []
    for i in range(num_layers):
        out += ['DNN/%s/layer%d/weights' % (input_name, i), 'DNN/%s/layer%d/biases' % (input_name, i)]
        if layer_norm:
            ln = 'LayerNorm' if i == 0 else 'LayerNorm_%d' % i
            out += ['DNN/%s/%s/beta' % (input_name, ln), 'DNN/%s/%s/gamma' % (input_name, ln)]
    return out + ['DNNDecoder/%s/outlayer/weights' % output_name, 'DNNDecoder/%s/outlayer/biases' % output_name]


def step(params, x, lens, targets, target_lens, context, num_layers, layer_norm=True, masks=None,
         input_name='features', output_name='alignments'):
    """(loss, {name: gradient}) of average_cross_entropy over the model, float64; params: {name: array}"""
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    h = stack_seq(splice(torch.tensor(np.asarray(x, np.float64)), context), lens)
    for i in range(num_layers):
        pre = 'DNN/%s/layer%d/' % (input_name, i)
        z = h @ p[pre + 'weights'] + p[pre + 'biases']
        if layer_norm:
            ln = 'DNN/%s/%s/' % (input_name, 'LayerNorm' if i == 0 else 'LayerNorm_%d' % i)
            h = relu_layer_norm(z, p[ln + 'gamma'], p[ln + 'beta'])
        else:
            h = torch.relu(z)
        if masks is not None:
            h = h * torch.from_numpy(masks[i])
    enc = unstack_seq(h, lens)
    pre = 'DNNDecoder/%s/outlayer/' % output_name
    logits = enc @ p[pre + 'weights'] + p[pre + 'biases']
    B, Tm, C = logits.shape
    logp = torch.log_softmax(logits, -1)
    tg = torch.tensor(np.asarray(targets)[:, :Tm].astype(np.int64))
    nll = -logp.gather(2, tg[:, :, None])[:, :, 0]
    mask = torch.arange(Tm)[None, :] < torch.tensor(np.asarray(lens))[:, None]
    per = (nll * mask).sum(1) / torch.tensor(np.asarray(target_lens, np.float64))
    loss = per.mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}
