"""AlignmentDecoder (reference: nabu/neuralnetworks/decoders/alignment_decoder.py:10-104): the pseudo
log-likelihoods of the HMM states for a Kaldi decoder,
    loglikes = log(softmax(logits)) - log(prior),
with prior = np.load(conf['prior']), or a uniform prior (and the reference's warning) when that file does not
exist.  One kernel per batch (nabu_log_softmax_prior_f32); log(prior) is uploaded once per decoder.

`write` appends one Kaldi binary matrix per utterance, cut to its length, to <directory>/<output>/loglikes.ark and
a line `name ark:offset` to feats.scp, byte for byte as the reference's arkwrite: the key, then (offset points
here) NUL 'B' 'F' 'M' ' ', int8 4, int32 rows, int8 4, int32 cols, rows x cols float32, little-endian.  Quirk kept
from the reference: no space between the key and the NUL (Kaldi's own writer puts one there)."""
import os
import struct

import numpy as np
import torch

from nabu_amd import ops
from nabu_amd.autodiff import SeqLen
from nabu_amd.neuralnetworks.decoders import decoder
from nabu_amd.processing import ngram_lm


class AlignmentDecoder(decoder.Decoder):
    '''gets the HMM state posteriors'''

    def __init__(self, conf, model):
        super(AlignmentDecoder, self).__init__(conf, model)
        ngram_lm.refuse_keys(self.conf, 'AlignmentDecoder')
        self._logprior = None

    def log_prior(self):
        '''log(prior) as float64 on the host (alignment_decoder.py:40-49)'''
        if os.path.exists(self.conf['prior']):
            prior = np.load(self.conf['prior'])
        else:
            print('WARNING could not find prior in file %s using uniform'
                  ' prior' % self.conf['prior'])
            output_dim = list(self.model.output_dims.values())[0]
            prior = np.ones([output_dim]) / output_dim
        return np.log(np.asarray(prior, np.float64))

    def __call__(self, inputs, input_seq_length):
        '''Returns {output: (loglikes [B,T,C] device tensor, lengths [B] int32)}'''
        with torch.no_grad():
            logits, logits_seq_length = self.model(inputs, input_seq_length, targets=[], target_seq_length=[],
                                                   is_training=False)
            x = list(logits.values())[0]                    # logits.values()[0] of the reference
            if self._logprior is None:
                self._logprior = torch.from_numpy(self.log_prior().astype(np.float32)).to(x.device)
            outputs = {}
            for o in logits:
                lens = SeqLen.wrap(logits_seq_length[o], x.device)
                outputs[o] = (ops.log_softmax_prior(x.contiguous(), lens.dev, self._logprior), lens.host)
        return outputs

    def write(self, outputs, directory, names):
        '''append every utterance's matrix to <directory>/<output>/loglikes.ark (+ feats.scp)'''
        for o in outputs:
            if not os.path.isdir(os.path.join(directory, o)):
                os.makedirs(os.path.join(directory, o))
            loglikes = outputs[o][0].cpu().numpy()
            lengths = decoder.host_lengths(outputs[o][1])
            scp_file = os.path.join(directory, o, 'feats.scp')
            ark_file = os.path.join(directory, o, 'loglikes.ark')
            for i in range(loglikes.shape[0]):
                arkwrite(scp_file, ark_file, names[i], loglikes[i, :lengths[i]])

    def update_evaluation_loss(self, loss, outputs, references, reference_seq_length):
        raise Exception('AlignmentDecoder can not be used to validate')


def arkwrite(scp_file, ark_file, name, array):
    '''append `array` [rows, cols] float32 to ark_file under key `name` and its `name ark_file:offset` line to
    scp_file (alignment_decoder.py:89-104); offset = the position of the NUL after the key'''
    array = np.ascontiguousarray(array, dtype='<f4')
    rows, cols = array.shape
    with open(ark_file, 'ab') as ark_fid:
        ark_fid.write(name.encode())
        pos = ark_fid.tell()
        ark_fid.write(struct.pack('<xcccc', b'B', b'F', b'M', b' '))
        ark_fid.write(struct.pack('<bi', 4, rows))
        ark_fid.write(struct.pack('<bi', 4, cols))
        ark_fid.write(array.tobytes())
    with open(scp_file, 'a') as scp_fid:
        scp_fid.write('%s %s:%s\n' % (name, ark_file, pos))
