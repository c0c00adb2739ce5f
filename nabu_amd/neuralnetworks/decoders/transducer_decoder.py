"""TransducerDecoder (not in the reference): greedy or beam search with an RNN transducer model (decoder = transducer),
all utterances of the batch in lock-step on the device.

Every iteration is one nabu_transducer_greedy_step launch — each row takes the arg-max of f[b, t_pos] + g_row[b]; the
blank moves it to the next frame, a label is appended — then one step of the prediction network for the rows that
emitted (the others keep their state: `emit` is the step's seq_len) and the output product that gives the next g_row.
A row is finished after at most T' + max_steps iterations; every 32 iterations the host reads ONE word saying whether
all rows are, and does not synchronise otherwise.

With beam_width = W in 2..32 the search is the alignment-length synchronous beam search (Saon, Tueske and Audhkhasi
2020; the definition is nabu_transducer_beam_step's in include/nabu_hip.h): B W rows of the prediction network, and per
iteration one nabu_transducer_beam_step launch for the whole beam of every utterance — hypotheses that spell the same
labels meet there and their probabilities are added — then predict_reorder (the survivors take their parents' state)
and predict_step (those that emitted advance).  An utterance is done when no hypothesis of its beam is active, after at
most T' + max_steps iterations; every 32 iterations the host reads ONE word saying whether all are.  The result is the
best completed hypothesis; self.nbest keeps all W of them.  Language-model fusion and score normalisation are out of
scope here.

With emission_times = True (an extension key: absent from the defaults, off when absent) the recognised labels — the
greedy path's, or the best final's of the beam search — are then aligned to the SAME f (nabu_transducer_align): the
prediction network runs teacher-forced on the recognised ids for g, the encoder does not run again.  `write` adds
<output>.ctm — name 1 start duration symbol confidence per label, as ctc_decoder does for `timestamps`: a label starts
at its emission frame and lasts until the next label's (the end of the utterance for the last), at least one frame — a
convention, a transducer emits at instants (transducer_alignment_decoder.py); confidence = exp(log-probability of the
label at its emission node); in encoded frames, or in seconds with frame_seconds > 0, which is honoured only together
with the key.  The forced alignment is the BEST path of the recognised labels, which need not be the path the greedy
search walked.  The key is not called `timestamps`: that one stays refused.

conf: <output>_alphabet as for ctc_decoder; max_steps (required): the most labels an utterance gets; beam_width
(optional, 1..32; absent or 1: the greedy search); emission_times, frame_seconds (optional)."""
import torch

from nabu_amd import ops
from nabu_amd import variables as vs
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.decoders import ctc_alignment_decoder, ctc_decoder, decoder, transducer_alignment_decoder
from nabu_amd.neuralnetworks.models.ed_decoders import transducer

POLL = 32                 # iterations between two reads of the "all rows finished" word
REFUSED = ('lm_file', 'lm_weight', 'insertion_bonus', 'ctc_weight', 'timestamps', 'frame_seconds')


def emission_times_key(conf):
    """the `emission_times` key of the [decoder] section (an extension key: absent from the defaults, off when absent)"""
    text = str(conf.get('emission_times', 'False')).strip()
    if text not in ('True', 'False'):
        raise ValueError('emission_times must be True or False, got %r' % text)
    return text == 'True'


class TransducerDecoder(decoder.Decoder):
    '''greedy or beam transducer search; the outputs, the written files and the error rate are CTCDecoder's'''

    def __init__(self, conf, model):
        super(TransducerDecoder, self).__init__(conf, model)
        if not isinstance(model.decoder, transducer.Transducer):
            raise ValueError('transducer_decoder searches with a transducer model (decoder = transducer in the model\'s '
                             '[decoder] section), got %s' % type(model.decoder).__name__)
        self.emission_times = emission_times_key(self.conf)
        for key in REFUSED:
            if key in self.conf and not (key == 'frame_seconds' and self.emission_times):
                raise ValueError('transducer_decoder searches with the model alone: the key %s is not supported' % key)
        self.max_steps = int(self.conf['max_steps'])
        if self.max_steps < 1:
            raise ValueError('max_steps must be positive, got %d' % self.max_steps)
        width = self.conf.get('beam_width', '1').strip()
        if not width.isdigit() or not 1 <= int(width) <= 32:
            raise ValueError('beam_width must be an integer in 1..32, got %r' % width)
        self.beam_width = int(width)
        self.alphabets = {o: self.conf['%s_alphabet' % o].split(' ') for o in model.output_names}
        self.frame_seconds = ctc_alignment_decoder.frame_seconds_key(self.conf) if self.emission_times else 0.0

    def __call__(self, inputs, input_seq_length):
        '''Returns {output: (ids [B,max_steps] int32 padded with -1, lengths [B] int32)}, as CTCDecoder does; self.scores
        keeps {output: log p of the path taken [B]} (beam search: of the best hypothesis, all its alignments that the
        beam kept added up) and, for the beam search, self.nbest {output: (ids [B,W,max_steps], lengths [B,W], log p
        [B,W])}: the completed hypotheses, best first, lengths -1 where there are fewer than W.  With emission_times =
        True the tuple goes on with (seg [B,max_steps,2], conf [B,max_steps], score [B]): first frame and last frame + 1
        of every label by the module's convention, ops.transducer_align's conf and score'''
        net = self.model.decoder
        outputs, self.scores, self.nbest = {}, {}, {}
        with torch.no_grad():
            logits, logit_len = self.model(inputs, input_seq_length, targets=[], target_seq_length=[], is_training=False)
            for o in self.model.output_names:
                f = logits[o].contiguous()
                B, T, C = f.shape
                dev, S = f.device, self.max_steps
                lens = SeqLen.wrap(logit_len[o], dev)
                if self.beam_width > 1:
                    outputs[o], self.scores[o], self.nbest[o] = self._beam(net, o, f, lens)
                    if self.emission_times:
                        outputs[o] += self._emission_times(net, o, f, lens, *outputs[o])
                    continue
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
                if self.emission_times:
                    outputs[o] += self._emission_times(net, o, f, lens, ids, out_len)
        return outputs

    def _emission_times(self, net, o, f, lens, ids, out_len):
        '''(seg [B,max_steps,2], conf [B,max_steps], score [B]) of the recognised labels aligned to f.  The labels are cut
        to the longest row (one host read) so that the lattice is no wider than it must be'''
        B, S = ids.shape
        none = out_len < 0                                   # (the beam search's utterance without a completed hypothesis)
        out_len = out_len.clamp(min=0)
        L = int(out_len.max().item())
        labels = ids[:, :L].clamp(min=0).contiguous()
        with vs.as_default(self.model.store):
            g = net.predict_sequence(o, labels, out_len)
        _, frame, conf, score, _ = ops.transducer_align(f, g, lens.dev, labels if L else None, out_len)
        seg = torch.full((B, S, 2), -1, dtype=torch.int32, device=f.device)
        cf = torch.zeros((B, S), dtype=torch.float32, device=f.device)
        seg[:, :L] = transducer_alignment_decoder.emission_segments(frame, out_len, lens.dev)
        cf[:, :L] = conf
        return seg, cf, score.masked_fill(none, float('-inf'))          # (-inf: `write` gives the row no lines)

    def _beam(self, net, o, f, lens):
        '''((ids [B,max_steps], lengths [B]), log p [B], (all finals)) of output o'''
        B, T, C = f.shape
        dev, S, W = f.device, self.max_steps, self.beam_width
        beam = ops.transducer_beam_state(B, W, S, dev)
        with vs.as_default(self.model.store):
            state = net.predict_start(o, B * W, dev)
        # the empty history: every row reads the start symbol (the blank's class)
        g_rows = net.predict_step(state, torch.full((B * W,), C - 1, dtype=torch.int32, device=dev),
                                  torch.ones(B * W, dtype=torch.int32, device=dev))
        for it in range(T + S):
            ops.transducer_beam_step(it, f, g_rows, lens.dev, beam)
            net.predict_reorder(state, beam.parent)
            g_rows = net.predict_step(state, beam.last_id.view(B * W), beam.emit.view(B * W))
            if it % POLL == POLL - 1 and bool((beam.out_len < 0).all().item()):
                break
        return ((beam.fin_ids[:, 0].contiguous(), beam.fin_len[:, 0].contiguous()), beam.fin_score[:, 0].contiguous(),
                (beam.fin_ids, beam.fin_len, beam.fin_score))

    # one line "<name> <symbols>" per utterance; sum of edit distances / number of reference labels
    write = ctc_decoder.CTCDecoder.write
    update_evaluation_loss = ctc_decoder.CTCDecoder.update_evaluation_loss
