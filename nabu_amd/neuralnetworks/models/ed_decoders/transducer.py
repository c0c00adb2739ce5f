"""RNN transducer decoder (Graves 2012, "Sequence Transduction with Recurrent Neural Networks"; not in the reference):
a transcription network — one linear layer on the first encoded input — and a prediction network — a unidirectional
LSTM over the label history followed by a linear layer.  Their logits f [B,T,C] and g [B,U1,C] meet in the additive
joint h[t,u,k] = f[t,k] + g[u,k], which only the loss (loss = transducer, nabu_transducer_loss_grad) and the search
(decoder = transducer_decoder, nabu_transducer_greedy_step or, with beam_width, nabu_transducer_beam_step) evaluate: h is
never materialised.

Variables of output o (blank = start symbol = C-1, the class `trainlabels = 1` adds):
    Transducer/o/transcription/{weights,biases}                      dnn_decoder.linear
    Transducer/o/prediction/layer<l>/lstm_cell/{kernel,bias}         [in+U,4U], gates i,j,f,o, forget bias 1
    Transducer/o/prediction/outlayer/{weights,biases}                dnn_decoder.linear on the top layer's outputs

With targets the prediction network reads the start symbol followed by the targets, one-hot, for U1 = Lmax + 1 steps
with seq_len = target_len + 1: a step chain of nabu_lstm_cell_fwd, the first layer's input product being the row gather
of that kernel; its backward pass is one tape node.  Without targets (every inference decoder calls the model with
targets = []) only f is returned, and predict_start / predict_step run the network one label at a time; the beam search
runs B W rows and moves their states to the survivors with predict_reorder."""
import torch

from nabu_amd import ops as hip
from nabu_amd import variables as vs
from nabu_amd.autodiff import record, SeqLen
from nabu_amd.neuralnetworks.models.ed_decoders import dnn_decoder, ed_decoder

PRED = '_pred'          # suffix of the prediction logits' key, beside <output> (as <output>_ctc of the CTC head)


class Transducer(ed_decoder.EDDecoder):
    '''transcription and prediction network of an RNN transducer with the additive joint'''

    def __init__(self, conf, output_dims, constraint, name=None):
        super(Transducer, self).__init__(conf, output_dims, constraint, name)
        self.num_layers, self.num_units = int(self.conf['num_layers']), int(self.conf['num_units'])
        if self.num_layers < 1 or self.num_units < 1:
            raise ValueError('transducer: num_layers and num_units must be positive, got %d and %d'
                             % (self.num_layers, self.num_units))

    def _net(self, C):
        '''the prediction network's variables (inside the output's scope): [(kernel, bias)] per layer'''
        U, layers = self.num_units, []
        with vs.variable_scope('prediction'):
            for l in range(self.num_layers):
                with vs.variable_scope('layer%d/lstm_cell' % l):
                    layers.append((vs.get_variable('kernel', [(C if l == 0 else U) + U, 4 * U]),
                                   vs.get_variable('bias', [4 * U], vs.zeros)))
        return layers

    def _decode(self, encoded, encoded_seq_length, targets, target_seq_length, is_training):
        outputs, output_seq_length = {}, {}
        first = list(encoded.keys())[0]
        for o in self.output_dims:
            C = self.output_dims[o]
            with vs.variable_scope(o):
                outputs[o] = dnn_decoder.linear(encoded[first], C, 'transcription')
                output_seq_length[o] = encoded_seq_length[first]
                layers = self._net(C)
                if targets:
                    tsl = SeqLen.wrap(target_seq_length[o], outputs[o].device)
                    top = self._teacher_forced(layers, C, targets[o], tsl)
                    with vs.variable_scope('prediction'):
                        g_steps = dnn_decoder.linear(top, C, 'outlayer')                 # [U1,B,C]
                    g = g_steps.transpose(0, 1).contiguous()                             # batch-major, as f
                    record([g_steps], [g], lambda dg: [dg.transpose(0, 1).contiguous()])
                    outputs[o + PRED] = g
                    output_seq_length[o + PRED] = SeqLen(tsl.host + 1, dev_tensor=tsl.dev + 1)
                else:
                    with vs.variable_scope('prediction/outlayer'):                       # (the variables exist either way)
                        vs.get_variable('weights', [self.num_units, C])
                        vs.get_variable('biases', [C], vs.zeros)
        return outputs, output_seq_length, ()

    def _teacher_forced(self, layers, C, targets, tsl):
        '''the top layer's outputs [U1,B,U] (step-major) for the histories start, start + targets[:1], ...; steps from
        target_len + 1 on copy their state through'''
        U, dev = self.num_units, tsl.dev.device
        targets = torch.as_tensor(targets).to(dev)
        B, Lmax = targets.shape
        U1 = Lmax + 1
        seq_len = (tsl.dev + 1).to(torch.int32)
        # ids [U1,B]: what the network reads at step u (kept inside the kernel's rows; the loss reports a bad label)
        ids = torch.cat([torch.full((1, B), C - 1, dtype=torch.int32, device=dev),
                         targets.to(torch.int32).t().clamp(0, C - 1)], 0).contiguous()
        saved, below = [], None
        for l, (K, bias) in enumerate(layers):
            n_in = C if l == 0 else U
            Wx, Wh = K.data[:n_in], K.data[n_in:]
            z = torch.empty((U1, B, 4 * U), dtype=torch.float32, device=dev)
            if l:                      # the input products of all steps: one product
                hip.gemm(below.view(U1 * B, U), Wx, z.view(U1 * B, 4 * U))
            acts = torch.empty_like(z)
            c = torch.zeros((U1 + 1, B, U), dtype=torch.float32, device=dev)       # [0]: the zero state
            h = torch.zeros((U1 + 1, B, U), dtype=torch.float32, device=dev)
            for u in range(U1):
                hip.gemm(h[u], Wh, z[u], beta=1.0 if l else 0.0)
                hip.lstm_cell_fwd(u, seq_len, z[u], bias.data, Wx if l == 0 else None, ids[u] if l == 0 else None,
                                  c[u], h[u], acts[u], c[u + 1], h[u + 1])
            saved.append((acts, c, h, below))
            below = h[1:]
        top = below

        def backward(dtop):
            d_out = dtop.contiguous()                                  # [U1,B,U]: gradient of the layer's outputs
            for l in reversed(range(len(layers))):
                K, bias = layers[l]
                acts, c, h, x = saved[l]
                n_in = C if l == 0 else U
                for v in (K, bias):
                    if v.grad is None:
                        v.grad = torch.zeros_like(v.data)
                dz = torch.empty((U1, B, 4 * U), dtype=torch.float32, device=dev)
                dh = torch.zeros((B, U), dtype=torch.float32, device=dev)          # through the recurrence
                dc = torch.zeros((2, B, U), dtype=torch.float32, device=dev)
                for u in reversed(range(U1)):
                    hip.lstm_cell_bwd(u, seq_len, acts[u], c[u + 1], c[u], d_out[u], dh, dc[u & 1], dz[u], dc[1 - (u & 1)])
                    if u:
                        hip.gemm(dz[u], K.data[n_in:], dh, trans_b=True)          # into step u-1: dz[u] Wh^T
                dz2 = dz.view(U1 * B, 4 * U)
                # the weight gradients: ONE product over the stacked steps each
                hip.gemm(h[:U1].view(U1 * B, U), dz2, K.grad[n_in:], trans_a=True)
                hip.colsum(dz2, bias.grad)
                if l:
                    hip.gemm(x.reshape(U1 * B, U), dz2, K.grad[:n_in], trans_a=True)
                    d_out = torch.empty((U1, B, U), dtype=torch.float32, device=dev)
                    hip.gemm(dz2, K.data[:n_in], d_out.view(U1 * B, U), trans_b=True)
                else:                  # one-hot inputs: the input kernel's rows gather the steps that read them
                    hip.scatter_rows(ids.view(U1 * B), dz2, K.grad[:n_in])
            return []
        record([], [top], backward, params=tuple(v for pair in layers for v in pair))
        return top

    def predict_sequence(self, o, targets, target_seq_length):
        '''the prediction logits g [B,Lmax+1,C] of output o for the histories of targets [B,Lmax] — what the model
        returns as <output>_pred when it is called with targets — without running the encoder (transducer_decoder aligns
        what it has recognised to the f it already has).  Call with the model's store as the default.'''
        C = self.output_dims[o]
        with vs.variable_scope(self.scope), vs.variable_scope(o):
            layers = self._net(C)
            top = self._teacher_forced(layers, C, targets, SeqLen.wrap(target_seq_length, targets.device))
            with vs.variable_scope('prediction'):
                g_steps = dnn_decoder.linear(top, C, 'outlayer')                         # [U1,B,C]
        return g_steps.transpose(0, 1).contiguous()

    # ------------------------------------------------------------------ one label at a time (transducer_decoder)
    def predict_start(self, o, B, device):
        '''the search state of output o for B rows: the variables, zero LSTM states and the step's buffers.  Call with
        the model's store as the default (vs.as_default(model.store)).'''
        C, U = self.output_dims[o], self.num_units
        with vs.variable_scope(self.scope), vs.variable_scope(o):
            layers = self._net(C)
            with vs.variable_scope('prediction/outlayer'):
                W, b = vs.get_variable('weights', [U, C]), vs.get_variable('biases', [C], vs.zeros)

        def buf(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=device)
        return dict(C=C, layers=layers, W=W, b=b, z=buf(B, 4 * U), acts=buf(B, 4 * U), g=buf(B, C),
                    c=[[buf(B, U), buf(B, U)] for _ in layers], h=[[buf(B, U), buf(B, U)] for _ in layers])

    def predict_step(self, state, last_id, emit):
        '''rows with emit[b] = 1 read last_id[b] and advance, the others keep their state (emit is the seq_len of
        nabu_lstm_cell_fwd at step 0); returns the prediction logits g_row [B,C] of every row's history'''
        U = self.num_units
        x = None
        for l, (K, bias) in enumerate(state['layers']):
            n_in = state['C'] if l == 0 else U
            c, h = state['c'][l], state['h'][l]
            if l:
                hip.gemm(x, K.data[:n_in], state['z'])
            hip.gemm(h[0], K.data[n_in:], state['z'], beta=1.0 if l else 0.0)
            hip.lstm_cell_fwd(0, emit, state['z'], bias.data, K.data[:n_in] if l == 0 else None,
                              last_id if l == 0 else None, c[0], h[0], state['acts'], c[1], h[1])
            c.reverse()
            h.reverse()
            x = h[0]
        hip.gemm(x, state['W'].data, state['g'], bias=state['b'].data)
        return state['g']

    def predict_reorder(self, state, parent):
        '''the beam search's survivors take their parents' state: row b W + w of every layer's c and h becomes row
        b W + parent[b,w] (parent [B,W] int32 as nabu_transducer_beam_step writes it; the state has B W rows).  Call it
        before predict_step(state, last_id, emit) advances the rows that emitted.  The rows are gathered into the
        buffers the next predict_step would overwrite anyway, which then change places with the current ones — the
        same flip predict_step makes — so a parent may feed several children.'''
        B, W = parent.shape
        for l in range(len(state['layers'])):
            for bufs in (state['c'][l], state['h'][l]):
                U = bufs[0].shape[1]
                # nabu_beam_gather picks `old` or `fresh` by its stay argument: with both the same tensor it is a
                # plain gather, and any int32 array serves as stay
                hip.check(hip._hip.lib().nabu_beam_gather(B, W, U, hip.ptr(bufs[0]), hip.ptr(bufs[0]), hip.ptr(parent),
                                                          hip.ptr(parent), hip.ptr(bufs[1]), hip.stream()),
                          'nabu_beam_gather')
                bufs.reverse()

    def zero_state(self, encoded_dim, batch_size):
        return ()
