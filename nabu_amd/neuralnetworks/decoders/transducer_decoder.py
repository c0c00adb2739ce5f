"""TransducerDecoder (not in the reference): greedy search with an RNN transducer model (decoder = transducer), all
utterances of the batch in lock-step on the device.

Every iteration is one nabu_transducer_greedy_step launch — each row takes the arg-max of f[b, t_pos] + g_row[b]; the
blank moves it to the next frame, a label is appended — then one step of the prediction network for the rows that
emitted (the others keep their state: `emit` is the step's seq_len) and the output product that gives the next g_row.
A row is finished after at most T' + max_steps iterations; every 32 iterations the host reads ONE word saying whether
all rows are, and does not synchronise otherwise.  Beam search and language-model fusion are out of scope here.

conf: <output>_alphabet as for ctc_decoder; max_steps (required): the most labels an utterance gets."""
import torch

from nabu_amd import ops
from nabu_amd import variables as vs
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.decoders import ctc_decoder, decoder
from nabu_amd.neuralnetworks.models.ed_decoders import transducer

POLL = 32                 # iterations between two reads of the "all rows finished" word
REFUSED = ('lm_file', 'lm_weight', 'insertion_bonus', 'ctc_weight', 'timestamps', 'frame_seconds')


class TransducerDecoder(decoder.Decoder):
    '''greedy transducer search; the outputs, the written files and the error rate are CTCDecoder's'''

    def __init__(self, conf, model):
        super(TransducerDecoder, self).__init__(conf, model)
        if not isinstance(model.decoder, transducer.Transducer):
            raise ValueError('transducer_decoder searches with a transducer model (decoder = transducer in the model\'s '
                             '[decoder] section), got %s' % type(model.decoder).__name__)
        for key in REFUSED:
            if key in self.conf:
                raise ValueError('transducer_decoder is a plain greedy search: the key %s is not supported' % key)
        self.max_steps = int(self.conf['max_steps'])
        if self.max_steps < 1:
            raise ValueError('max_steps must be positive, got %d' % self.max_steps)
        self.alphabets = {o: self.conf['%s_alphabet' % o].split(' ') for o in model.output_names}

    def __call__(self, inputs, input_seq_length):
        '''Returns {output: (ids [B,max_steps] int32 padded with -1, lengths [B] int32)}, as CTCDecoder does; self.scores
        keeps {output: log p of the path taken [B]}'''
        net = self.model.decoder
        outputs, self.scores = {}, {}
        with torch.no_grad():
            logits, logit_len = self.model(inputs, input_seq_length, targets=[], target_seq_length=[], is_training=False)
            for o in self.model.output_names:
                f = logits[o].contiguous()
                B, T, C = f.shape
                dev, S = f.device, self.max_steps
                lens = SeqLen.wrap(logit_len[o], dev)
                t_pos, out_len, emit, last_id = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4))
                ids = torch.empty((B, S), dtype=torch.int32, device=dev)
                score = torch.empty(B, dtype=torch.float32, device=dev)
                with vs.as_default(self.model.store):
                    state = net.predict_start(o, B, dev)
                # the empty history: every row reads the start symbol (the blank's class)
                g_row = net.predict_step(state, torch.full((B,), C - 1, dtype=torch.int32, device=dev),
                                         torch.ones(B, dtype=torch.int32, device=dev))
                for it in range(T + S):
                    ops.transducer_greedy_step(it, f, g_row, lens.dev, t_pos, out_len, ids, emit, last_id, score)
                    g_row = net.predict_step(state, last_id, emit)
                    if it % POLL == POLL - 1 and bool(((t_pos >= lens.dev) | (out_len >= S)).all().item()):
                        break
                outputs[o] = (ids, out_len)
                self.scores[o] = score
        return outputs

    # one line "<name> <symbols>" per utterance; sum of edit distances / number of reference labels
    write = ctc_decoder.CTCDecoder.write
    update_evaluation_loss = ctc_decoder.CTCDecoder.update_evaluation_loss
