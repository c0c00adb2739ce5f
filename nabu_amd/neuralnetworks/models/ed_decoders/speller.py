"""The Speller decoder of the LAS architecture
(reference: nabu/neuralnetworks/models/ed_decoders/speller.py:13-69)."""
from nabu_amd.neuralnetworks.components import attention
from nabu_amd.neuralnetworks.components import rnn_cell as rnn_cell_lib
from nabu_amd.neuralnetworks.models.ed_decoders import rnn_decoder


class Speller(rnn_decoder.RNNDecoder):
    '''a speller decoder for the LAS architecture'''

    def create_cell(self, encoded, encoded_seq_length, is_training):
        '''MultiRNNCell(LSTMCell x num_layers, output dropout when training) ->
        AttentionWrapper(output_attention=False) -> AttentionProjectionWrapper'''
        keep = float(self.conf['dropout'])
        rnn_cells = [rnn_cell_lib.LSTMCell(
            num_units=int(self.conf['num_units']),
            output_keep_prob=keep if (keep < 1 and is_training) else 1.0)
            for _ in range(int(self.conf['num_layers']))]
        # one mechanism per encoded input, in the order of `encoded` (reference speller.py:49-61)
        mechanisms = [attention.factory(conf=self.conf, num_units=rnn_cells[-1].num_units, encoded=encoded[e],
                                        encoded_seq_length=encoded_seq_length[e], index=m)
                      for m, e in enumerate(encoded)]
        cell = rnn_cell_lib.AttentionWrapper(cells=rnn_cells, attention_mechanism=mechanisms)
        return rnn_cell_lib.AttentionProjectionWrapper(
            cell=cell, output_dim=list(self.output_dims.values())[0])
