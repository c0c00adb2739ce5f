"""CTCAlignmentDecoder: forced alignment of a transcription to its audio with a CTC model (no counterpart in the
reference).  The best path through the label lattice the CTC loss sums over — nabu_ctc_align, one launch per batch
— gives every encoded frame its symbol and every label its first frame, its length and a confidence.

Logits.  A CTC-trained model (dnn_decoder on dblstm or listener) is aligned with its own logits.  A Speller with
ctc_head = True is aligned with the head's logits on the first encoded input; the end label is dropped from the
references, as joint training drops it (it is the head's blank).  A Speller without the head and the dnn encoder
(frame targets: there is nothing to align) are refused.

References.  needs_targets = True: the Recognizer reads a target section per model output (`<output> = <database
sections>` in [recognizer], as a trainer conf names its targets) and passes targets=, target_seq_length= to the call.

Files, under <directory>/<output>/, appended per batch:
  alignment      name and one symbol per ENCODED frame, the blank written as `blank_symbol`
  segments.ctm   name 1 start duration symbol confidence   per label; confidence = exp(mean log-probability over the
                 label's frames).  frame_seconds = 0 writes frame indices; a positive value is the duration of ONE
                 ENCODED FRAME in seconds.  A Listener's pyramid shortens time (every layer stacks `pyramid_steps`
                 frames: 10 ms features and three layers of 2 make 0.08) — the key is where the user says by how much;
                 it is not guessed from the model.
  scores         name and the path's log-probability
An utterance whose transcription does not fit its encoded length (or holds a label outside the alphabet) is reported
by name and written to none of the files; `misfit = raise` makes it an exception instead (loss_functions.
ctc_status_error, what training raises for such an utterance)."""
import math
import os

import torch

from nabu_amd import ops
from nabu_amd import variables as vs
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.decoders import decoder
from nabu_amd.processing import ngram_lm


def frame_seconds_key(conf):
    text = str(conf.get('frame_seconds', '0')).strip()
    try:
        value = float(text)
    except ValueError:
        raise ValueError('frame_seconds must be a number, got %r' % text)
    if not (value >= 0.0 and math.isfinite(value)):
        raise ValueError('frame_seconds must be finite and >= 0, got %r' % text)
    return value


def ctm_lines(name, seg, conf, symbols, frame_seconds):
    '''the ctm lines of one utterance: seg [L,2] frames, conf [L] mean log-probabilities, symbols [L]'''
    lines = []
    for (start, end), c, sym in zip(seg, conf, symbols):
        if frame_seconds > 0:
            when = '%.3f %.3f' % (start * frame_seconds, (end - start) * frame_seconds)
        else:
            when = '%d %d' % (start, end - start)
        lines.append('%s 1 %s %s %.4f\n' % (name, when, sym, math.exp(float(c))))
    return lines


class CTCAlignmentDecoder(decoder.Decoder):
    '''forced alignment; conf: <output>_alphabet, blank_symbol, frame_seconds, misfit
    (defaults/ctcalignmentdecoder.cfg)'''

    needs_targets = True

    def __init__(self, conf, model):
        super(CTCAlignmentDecoder, self).__init__(conf, model)
        ngram_lm.refuse_keys(self.conf, 'CTCAlignmentDecoder')
        if 'ctc_weight' in self.conf:
            raise ValueError('CTCAlignmentDecoder does not take ctc_weight: there is no search to weigh')
        encoder, ed_decoder = model.conf.get('encoder', 'encoder'), model.conf.get('decoder', 'decoder')
        if encoder == 'dnn':
            raise ValueError('CTCAlignmentDecoder needs a CTC model; the dnn encoder is trained on frame targets')
        if ed_decoder == 'dnn_decoder':
            self.head = False
            self.outputs = list(model.output_names)
        elif getattr(model.decoder, 'ctc_head', False):
            self.head = True
            self.outputs = list(model.output_names)[:1]       # the head belongs to the first output
        else:
            raise ValueError('CTCAlignmentDecoder needs CTC logits: a %s without a CTC head has none (set ctc_head = '
                             'True in the [decoder] section of the model and train with ctc_weight)' % ed_decoder)
        self.alphabets = {}
        for o in self.outputs:
            if '%s_alphabet' % o not in self.conf:
                raise ValueError('CTCAlignmentDecoder: no %s_alphabet in the [decoder] section' % o)
            self.alphabets[o] = self.conf['%s_alphabet' % o].split(' ')
        self.blank_symbol = self.conf['blank_symbol']
        self.frame_seconds = frame_seconds_key(self.conf)
        if self.conf['misfit'] not in ('report', 'raise'):
            raise ValueError('misfit must be report or raise, got %r' % self.conf['misfit'])
        self.raise_on_misfit = self.conf['misfit'] == 'raise'

    def _logits(self, inputs, input_seq_length):
        '''{output: (CTC logits [B,T,C], their lengths)}'''
        model = self.model
        if not self.head:
            logits, logit_len = model(inputs, input_seq_length, targets=[], target_seq_length=[], is_training=False)
            return {o: (logits[o], logit_len[o]) for o in self.outputs}
        with vs.as_default(model.store):
            encoded, encoded_len = model.encoder(inputs=inputs, input_seq_length=input_seq_length, is_training=False)
            with vs.variable_scope(model.decoder.scope):
                return {self.outputs[0]: model.decoder.ctc_logits(encoded, encoded_len)}

    def __call__(self, inputs, input_seq_length, targets=None, target_seq_length=None):
        '''Returns {output: (state [B,T], seg [B,L,2], conf [B,L], score [B], frames [B] (host), labels [B,L],
        label lengths [B])} — device tensors but for `frames`'''
        if targets is None or target_seq_length is None:
            raise ValueError('CTCAlignmentDecoder aligns references: call it with targets= and target_seq_length=')
        outputs = {}
        with torch.no_grad():
            for o, (lg, lens) in self._logits(inputs, input_seq_length).items():
                dev = lg.device
                lens = SeqLen.wrap(lens, dev)
                labels = torch.as_tensor(targets[o]).to(device=dev, dtype=torch.int32).contiguous()
                label_len = SeqLen.wrap(target_seq_length[o], dev).dev
                if self.head:
                    label_len = (label_len - 1).clamp_(min=0)
                label_len = label_len.to(torch.int32).contiguous()
                state, seg, conf, score, _ = ops.ctc_align(lg.contiguous(), lens.dev, labels, label_len,
                                                           raise_on_status=self.raise_on_misfit)
                outputs[o] = (state, seg, conf, score, lens.host, labels, label_len)
        return outputs

    def write(self, outputs, directory, names):
        for o, (state, seg, conf, score, frames, labels, label_len) in outputs.items():
            state, seg, conf, score = state.cpu().numpy(), seg.cpu().numpy(), conf.cpu().numpy(), score.cpu().numpy()
            labels, label_len = labels.cpu().numpy(), label_len.cpu().numpy()
            frames = decoder.host_lengths(frames)
            alphabet = self.alphabets[o]
            if not os.path.isdir(os.path.join(directory, o)):
                os.makedirs(os.path.join(directory, o))
            with open(os.path.join(directory, o, 'alignment'), 'a') as afid, \
                    open(os.path.join(directory, o, 'segments.ctm'), 'a') as cfid, \
                    open(os.path.join(directory, o, 'scores'), 'a') as sfid:
                for i, name in enumerate(names):
                    L = max(int(label_len[i]), 0)
                    if not math.isfinite(float(score[i])):
                        print('CTCAlignmentDecoder: %s is not aligned: its %d labels do not fit its %d encoded frames '
                              '(or a label is outside the alphabet)' % (name, L, int(frames[i])))
                        continue
                    symbols = [alphabet[j] for j in labels[i, :L]]
                    path = state[i, :int(frames[i])]
                    afid.write('%s %s\n' % (name, ' '.join(symbols[s >> 1] if s & 1 else self.blank_symbol for s in path)))
                    cfid.writelines(ctm_lines(name, seg[i, :L], conf[i, :L], symbols, self.frame_seconds))
                    sfid.write('%s %f\n' % (name, score[i]))

    def update_evaluation_loss(self, loss, outputs, references, reference_seq_length):
        raise Exception('CTCAlignmentDecoder can not be used to validate')
