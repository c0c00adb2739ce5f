"""EDDecoder base class (reference: models/ed_decoders/ed_decoder.py:9-136)."""
from abc import ABCMeta, abstractmethod

from nabu_amd import variables as vs
from nabu_amd.tools.default_conf import apply_defaults, defaults_path


def ctc_head_key(conf):
    """the `ctc_head` key of the [decoder] section (a build addition like the trainer's label_smoothing: absent from the
    defaults files, False when absent): a CTC output layer on the first encoded input beside the recurrent decoder"""
    text = str(conf.get('ctc_head', 'False')).strip()
    if text not in ('True', 'False'):
        raise ValueError('ctc_head must be True or False, got %r' % text)
    return text == 'True'


class EDDecoder(object, metaclass=ABCMeta):
    '''a general decoder for an encoder decoder system: converts the high level
    features into output logits'''

    supports_ctc_head = False          # the recurrent decoders do (rnn_decoder.py)

    def __init__(self, conf, output_dims, constraint, name=None):
        self.conf = dict(conf.items('decoder'))
        apply_defaults(self.conf, defaults_path(__file__, self))
        self.ctc_head = ctc_head_key(self.conf)
        if self.ctc_head and not self.supports_ctc_head:
            raise ValueError('ctc_head = True is for a recurrent attention decoder (speller); %s is no such decoder'
                             % type(self).__name__)
        self.outputs = list(output_dims.keys())
        self.output_dims = output_dims
        self.constraint = constraint
        self.scope = name or type(self).__name__

    def __call__(self, encoded, encoded_seq_length, targets, target_seq_length, is_training):
        '''Returns (logits dict, logit sequence length dict, final state)'''
        with vs.variable_scope(self.scope):
            return self._decode(encoded, encoded_seq_length, targets, target_seq_length, is_training)

    @abstractmethod
    def _decode(self, encoded, encoded_seq_length, targets, target_seq_length, is_training):
        '''create the variables and decode an entire sequence'''

    @abstractmethod
    def zero_state(self, encoded_dim, batch_size):
        '''the decoder zero state'''

    @property
    def variables(self):
        variables = vs.default_store().variables(self.scope + '/')
        if hasattr(self, 'wrapped'):
            variables += self.wrapped.variables
        return variables
