"""RandomDecoder (reference: nabu/neuralnetworks/decoders/random_decoder.py:9-191): one random sample per utterance
from the output distribution of the model's recurrent attention decoder.  The encoder runs once, then
rnn_decoder.sample (nabu_speller_sample) runs the cell free on its own draws on the device: the reference's
SampleEmbeddingHelper + BasicDecoder under dynamic_decode(maximum_iterations = max_steps).

The draws come from the device Philox stream of `ops.global_rng()`: after `ops.set_seed` a decode is reproducible.
A call takes max_steps offsets from that stream, one per step.

Evaluation = edit distance of sequences[:, :lengths - 1] against the references, divided by the reference lengths,
as the reference computes it (random_decoder.py:163-185).  `lengths` counts the end label, so `lengths - 1` drops it —
and it drops the last real label of a row that reached max_steps without drawing the end label.  That is the
reference's behaviour and is kept."""
import os

import torch

from nabu_amd import ops
from nabu_amd import variables as vs
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.decoders import decoder
from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder
from nabu_amd.processing import ngram_lm

# the sampling streams of the decoder calls are `offset * OFFSET_STRIDE + step` (as rnn_decoder.dynamic_decode's)
OFFSET_STRIDE = 1000003


class RandomDecoder(decoder.Decoder):
    '''a decoder that returns a random sample from the output distribution; conf: max_steps, alphabet
    (defaults/randomdecoder.cfg)'''

    def __init__(self, conf, model):
        super(RandomDecoder, self).__init__(conf, model)
        ngram_lm.refuse_keys(self.conf, 'RandomDecoder')
        self.alphabet = self.conf['alphabet'].split(' ')

    def __call__(self, inputs, input_seq_length):
        '''Returns {output: (labels [B,time] int32, zero beyond lengths; lengths [B] int32, which count the end
        label; logprobs [B])}.  As in the reference, `logprobs` is the summed sparse softmax cross-entropy of the
        sampled labels: a POSITIVE number, minus the log-probability of the sample.'''
        model = self.model
        output_name = list(model.output_dims.keys())[0]
        max_steps = int(self.conf['max_steps'])
        rng = nops.global_rng()
        seed, offset = rng.next()
        rng.offset += max_steps - 1          # one offset per step
        with torch.no_grad(), vs.as_default(model.store):
            encoded, encoded_seq_length = model.encoder(inputs=inputs, input_seq_length=input_seq_length,
                                                        is_training=False)
            # the decoder's own scope, so the cell's variables are the trained ones
            with vs.variable_scope(model.decoder.scope):
                cell = model.decoder.create_cell(encoded, encoded_seq_length, False)
                names = list(encoded.keys())
                labels, lengths, logprobs, _ = rnn_decoder.sample(
                    cell, [encoded[e] for e in names], [encoded_seq_length[e] for e in names], max_steps=max_steps,
                    seed=seed, offset=offset * OFFSET_STRIDE)
        return {output_name: (labels, lengths, logprobs)}

    def write(self, outputs, directory, names):
        '''one line "<name> <symbols>" per utterance appended to <directory>/<output>, cut at lengths'''
        for o, out in outputs.items():
            labels, lengths = out[0].cpu().numpy(), out[1].cpu().numpy()
            with open(os.path.join(directory, o), 'a') as fid:
                for i, name in enumerate(names):
                    text = ' '.join(self.alphabet[j] for j in labels[i, :lengths[i]])
                    fid.write('%s %s\n' % (name, text))

    def update_evaluation_loss(self, loss, outputs, references, reference_seq_length):
        '''label error rate of sequences[:, :lengths - 1] (the module docstring says what that drops) against the
        whole references, over the number of reference labels'''
        out = list(outputs.values())[0]
        sequences, lengths = out[0].contiguous(), out[1]
        dev = sequences.device
        if sequences.shape[1] == 0:
            sequences = torch.zeros((sequences.shape[0], 1), dtype=torch.int32, device=dev)
        ref = torch.as_tensor(list(references.values())[0]).to(torch.int32).to(dev)
        ref_len = SeqLen.wrap(list(reference_seq_length.values())[0], dev)
        errors = int(ops.edit_distance(sequences, (lengths - 1).contiguous(), ref, ref_len.dev).sum().item())
        self._fold(loss, errors, int(decoder.host_lengths(ref_len).sum()))
