"""A dense n-gram language model over the output labels, for fusion in both beam searches (ops.ctc_beam_search_lm,
ops.beam_prune_lm / rnn_decoder.beam_search(lm=...)).  Host side, NumPy float64; the device reads the float32 table.

Symbols.  0 .. C-2 are the labels, C-1 is the boundary: as a predicted symbol the end of the sequence, as a context
symbol the start.  It is the index the Speller uses for its start/end label and CTC for its blank, so one table serves
both decoders of a recipe.

Table.  logprobs[ctx, c], float32 [C^(n-1), C]: ctx is the previous n-1 symbols as a base-C number, the most recent
symbol least significant.  The context of the empty hypothesis is every digit C-1; next(ctx, c) = (ctx C + c) mod
C^(n-1).  For n = 1 the table has one row and ctx is 0.

Estimator.  Interpolated Witten-Bell in float64:
    p_k(c | h) = (count(h, c) + N1+(h) p_{k-1}(c | h')) / (count(h) + N1+(h)),
N1+(h) the number of distinct successors of h, h' = h without its oldest symbol; p_k(c | h) = p_{k-1}(c | h') where
count(h) = 0; p_0 uniform over the C symbols.  A sentence is padded with n-1 boundaries in front and one at the end;
count_k(h, c) is the number of positions (every label and the final boundary) whose k-1 predecessors are h and whose
symbol is c.  Every entry is positive and every row sums to 1.

File.  .npz with order, num_labels (= C), logprobs and alphabet (the C-1 label symbols)."""
import numpy as np

MAX_ENTRIES = 1 << 24       # C^n entries at most (64 MiB of float32): the limit of the device entry points as well


def check_size(order, num_labels):
    """the number of contexts C^(order-1); refuses order < 1 and tables above MAX_ENTRIES"""
    order, C = int(order), int(num_labels)
    if order < 1:
        raise ValueError('n-gram order must be at least 1, got %d' % order)
    if C < 2:
        raise ValueError('an n-gram needs at least one label and the boundary (num_labels >= 2), got %d' % C)
    if C ** order > MAX_ENTRIES:
        raise ValueError('a table of %d^%d = %d entries exceeds the limit of 2^24 = %d entries (64 MiB)'
                         % (C, order, C ** order, MAX_ENTRIES))
    return C ** (order - 1)


def _contexts(padded, k, C):
    """index of the k-1 symbols before each position >= front of `padded` (most recent least significant)"""
    ctx = np.zeros(len(padded), np.int64)
    for j in range(1, k):
        ctx[j:] += padded[:len(padded) - j].astype(np.int64) * C ** (j - 1)
    return ctx


def estimate(sentences, num_labels, order):
    """probabilities [C^(order-1), C] float64 of the interpolated Witten-Bell estimator; sentences: label sequences
    (iterables of ints in [0, C-2])"""
    C, n = int(num_labels), int(order)
    check_size(n, C)
    counts = [np.zeros((C ** (k - 1), C), np.float64) for k in range(1, n + 1)]
    for s in sentences:
        s = np.asarray(list(s), np.int64)
        if s.size and (s.min() < 0 or s.max() > C - 2):
            raise ValueError('label outside [0, %d] in %r' % (C - 2, s.tolist()))
        padded = np.concatenate([np.full(n - 1, C - 1, np.int64), s, [C - 1]])
        for k in range(1, n + 1):
            ctx = _contexts(padded, k, C)[n - 1:]
            np.add.at(counts[k - 1], (ctx, padded[n - 1:]), 1.0)
    p = np.full((1, C), 1.0 / C)                  # p_0, as the one-row table of an order-0 model
    for k in range(1, n + 1):
        cnt = counts[k - 1]
        tot = cnt.sum(1, keepdims=True)
        n1 = (cnt > 0).sum(1, keepdims=True).astype(np.float64)
        # h' = h without its oldest symbol: the k-2 most recent symbols, i.e. h mod C^(k-2)
        lower = p[np.arange(cnt.shape[0]) % p.shape[0]] if k > 1 else np.broadcast_to(p, cnt.shape)
        with np.errstate(invalid='ignore', divide='ignore'):
            inter = (cnt + n1 * lower) / (tot + n1)
        p = np.where(tot > 0, inter, lower)
    return p


class NgramLM(object):
    """order, num_labels (= C), logprobs float32 [C^(order-1), C], alphabet (list of the C-1 label symbols)"""

    def __init__(self, order, num_labels, logprobs, alphabet):
        self.order, self.num_labels = int(order), int(num_labels)
        nctx = check_size(self.order, self.num_labels)
        self.logprobs = np.ascontiguousarray(logprobs, np.float32)
        if self.logprobs.shape != (nctx, self.num_labels):
            raise ValueError('logprobs has shape %r, an order-%d model over %d symbols needs %r'
                             % (self.logprobs.shape, self.order, self.num_labels, (nctx, self.num_labels)))
        if not np.all(np.isfinite(self.logprobs)):
            raise ValueError('logprobs must be finite (every probability positive)')
        self.alphabet = [str(a) for a in alphabet]
        if len(self.alphabet) != self.num_labels - 1:
            raise ValueError('%d symbols in the alphabet, %d labels in the model' % (len(self.alphabet), self.num_labels - 1))
        self._device = {}

    @property
    def num_contexts(self):
        return self.logprobs.shape[0]

    def start_context(self):
        """the context of the empty hypothesis: every digit the boundary"""
        return self.num_contexts - 1

    def next(self, ctx, c):
        return (int(ctx) * self.num_labels + int(c)) % self.num_contexts

    def sequence_logprob(self, labels, end=True):
        """log p(labels [followed by the end]) in float64 from the float32 table"""
        ctx, total = self.start_context(), 0.0
        for c in list(labels) + ([self.num_labels - 1] if end else []):
            total += float(self.logprobs[ctx, c])
            ctx = self.next(ctx, c)
        return total

    def device_table(self, device):
        """the table on `device`, uploaded once per model object and device"""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.logprobs).to(device).contiguous()
        return self._device[key]

    def save(self, path):
        with open(path, 'wb') as fid:       # (a file object: np.savez would append .npz to a bare name)
            np.savez(fid, order=np.int64(self.order), num_labels=np.int64(self.num_labels), logprobs=self.logprobs,
                     alphabet=np.array(self.alphabet, dtype=np.str_))


def train(sentences, alphabet, order):
    """the model of label sequences over `alphabet` (list of the C-1 label symbols)"""
    C = len(alphabet) + 1
    return NgramLM(order, C, np.log(estimate(sentences, C, order)), alphabet)


def load(path, num_labels=None, alphabet=None):
    """read a model file; num_labels (the model's output dimension + 1) and alphabet (list of symbols), where given,
    must be the file's"""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ('order', 'num_labels', 'logprobs', 'alphabet') if k not in z.files]
        if missing:
            raise ValueError('%s is not an n-gram model file: no %s' % (path, ', '.join(missing)))
        order, C = int(z['order']), int(z['num_labels'])
        check_size(order, C)
        lm = NgramLM(order, C, z['logprobs'], [str(a) for a in z['alphabet']])
    if num_labels is not None and lm.num_labels != int(num_labels):
        raise ValueError('%s: num_labels is %d, the model has output dimension + 1 = %d' % (path, lm.num_labels, int(num_labels)))
    if alphabet is not None and lm.alphabet != [str(a) for a in alphabet]:
        raise ValueError('%s: the alphabet of the language model differs from the decoder\'s' % path)
    return lm


def read_text(path, alphabet):
    """label sequences of a normalised text file: lines `<utterance id> <symbol> <symbol> ...`"""
    index = {s: i for i, s in enumerate(alphabet)}
    sentences = []
    with open(path) as fid:
        for lineno, line in enumerate(fid, 1):
            parts = line.split()
            if not parts:
                continue
            try:
                sentences.append([index[s] for s in parts[1:]])
            except KeyError as e:
                raise ValueError('%s, line %d (%s): symbol %r is not in the alphabet' % (path, lineno, parts[0], e.args[0]))
    return sentences


# ---------------------------------------------------------------------------------------------------------------
# the decoders' extension keys (absent from every defaults file, off when absent)
def _number(conf, key, default, what):
    text = str(conf.get(key, default)).strip()
    try:
        v = float(text)
    except ValueError:
        raise ValueError('%s must be a number, got %r' % (key, text))
    if not np.isfinite(v) or (what == 'weight' and v < 0):
        raise ValueError('%s must be finite%s, got %r' % (key, ' and >= 0' if what == 'weight' else '', text))
    return v


def decoder_keys(conf, with_bonus):
    """(lm_file or None, lm_weight, insertion_bonus) of a decoder's conf dict.  lm_weight defaults to 1 with an
    lm_file; lm_weight or insertion_bonus without lm_file is refused, as is a bad number (the key is named)."""
    lm_file = str(conf.get('lm_file', '')).strip() or None
    for key in ('lm_weight', 'insertion_bonus'):
        if key in conf and (key != 'insertion_bonus' or with_bonus) and lm_file is None:
            raise ValueError('%s needs a language model: set lm_file in the [decoder] section' % key)
    if 'insertion_bonus' in conf and not with_bonus:
        raise ValueError('insertion_bonus is a key of the CTC decoder only')
    weight = _number(conf, 'lm_weight', '1' if lm_file else '0', 'weight')
    bonus = _number(conf, 'insertion_bonus', '0', 'bonus') if with_bonus else 0.0
    return lm_file, weight, bonus


def refuse_keys(conf, who):
    """decoders without a search over labels"""
    for key in ('lm_file', 'lm_weight', 'insertion_bonus'):
        if key in conf:
            raise ValueError('%s does not take %s: language model fusion is for the CTC and beam search decoders' % (who, key))
