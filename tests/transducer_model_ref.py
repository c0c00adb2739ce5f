"""The transducer recipe's model in float64 (importable without a GPU): the DBLSTM encoder, the transcription layer, the
prediction network on one-hot label histories and its output layer assembled from oracle.nabu_oracle (dblstm_fwd/bwd,
linear_fwd/bwd, lstm_dir_fwd/bwd), the loss and the greedy search from tests/transducer_ref.py.  Parameters travel as
{variable name: float64 array}, the names being the model's own."""
import numpy as np

from oracle import nabu_oracle as O
from tests import transducer_ref as tr

CELL = 'bidirectional_rnn/%s/layer_norm_basic_lstm_cell/%s'
ENC = 'DBLSTM/features/layer%d/'
PRED = 'Transducer/text/prediction/layer%d/lstm_cell/'
TRANS = 'Transducer/text/transcription/'
OUT = 'Transducer/text/prediction/outlayer/'


def params_of(state):
    return {k: np.asarray(v).astype(np.float64) for k, v in state.items()}


def counts(P):
    n_enc = len([k for k in P if k.startswith('DBLSTM/') and k.endswith(CELL % ('fw', 'kernel'))])
    n_pred = len([k for k in P if k.startswith('Transducer/text/prediction/layer') and k.endswith('kernel')])
    return n_enc, n_pred


def _enc_layers(P, n_enc):
    return [{'%s_%s' % (d, w): P[ENC % l + CELL % (d, w)] for d in ('fw', 'bw') for w in ('kernel', 'bias')}
            for l in range(n_enc)]


def transcription(P, x, lens):
    """f [B,T,C], encoded lengths and what the backward pass needs"""
    n_enc, _ = counts(P)
    e, el, caches = O.dblstm_fwd(np.asarray(x, np.float64), lens, _enc_layers(P, n_enc))
    return O.linear_fwd(e, P[TRANS + 'weights'], P[TRANS + 'biases']), el, (e, caches)


def prediction(P, ids, lens):
    """g [B,U,C] for the label histories ids [B,U] (the start symbol first), lens [B] steps each"""
    _, n_pred = counts(P)
    C = P[OUT + 'weights'].shape[1]
    h = np.eye(C)[np.clip(np.asarray(ids, np.int64), 0, C - 1)]
    caches = []
    for l in range(n_pred):
        h, c = O.lstm_dir_fwd(h, np.asarray(lens), P[PRED % l + 'kernel'], P[PRED % l + 'bias'], False)
        caches.append(c)
    return O.linear_fwd(h, P[OUT + 'weights'], P[OUT + 'biases']), (h, caches)


def step(P, batch):
    """(mean nll, {name: gradient}) of one batch"""
    y = np.asarray(batch['targets']['text'])
    yl = np.asarray(batch['target_seq_length']['text'])
    B = y.shape[0]
    C = P[OUT + 'weights'].shape[1]
    f, el, (e, enc_caches) = transcription(P, batch['inputs']['features'], batch['input_seq_length']['features'])
    ids = np.concatenate([np.full((B, 1), C - 1, np.int64), y], 1)
    g, (h, pred_caches) = prediction(P, ids, yl + 1)
    nll, df, dg, status = tr.loss_grad(f, g, el, y, yl)
    assert status == 0
    G = {}
    de, G[TRANS + 'weights'], G[TRANS + 'biases'] = O.linear_bwd(df / B, e, P[TRANS + 'weights'])
    _, eg = O.dblstm_bwd(de, enc_caches)
    for l, gl in enumerate(eg):
        for d in ('fw', 'bw'):
            for w in ('kernel', 'bias'):
                G[ENC % l + CELL % (d, w)] = gl['%s_%s' % (d, w)]
    dh, G[OUT + 'weights'], G[OUT + 'biases'] = O.linear_bwd(dg / B, h, P[OUT + 'weights'])
    for l in reversed(range(len(pred_caches))):
        dh, G[PRED % l + 'kernel'], G[PRED % l + 'bias'] = O.lstm_dir_bwd(dh, pred_caches[l])
    return nll.mean(), G


def adam(P, G, M, V, t, lr=1e-3):
    """one clip + Adam update of every parameter, in place in the three dicts"""
    for k in P:
        P[k], M[k], V[k] = O.clip_adam_update(P[k], G[k], M.get(k, np.zeros_like(P[k])), V.get(k, np.zeros_like(P[k])), t, lr)


def greedy(P, x, lens, S):
    """the restatement's greedy search on the float64 forward pass: (ids, out_len, t_pos, score, margins)"""
    f, el, _ = transcription(P, x, lens)
    C = f.shape[2]

    def g_fn(b, ids):
        hist = np.concatenate([[C - 1], ids]).astype(np.int64)[None, :]
        return prediction(P, hist, [hist.shape[1]])[0][0, -1]
    return tr.greedy_search(f, el, S, g_fn, f.shape[1] + S) + (f, el)
