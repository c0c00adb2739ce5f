"""Timing of one iteration of the transducer's beam search (nabu_transducer_beam_step, csrc/transducer_beam.hip) against
two launches IN THE SAME RUN on the same operands, at [32, 125, 40], S = 50, W = 8 and W = 16:
    nabu_beam_prune at the same B, W, C — the project's kernel for the comparable job, log-softmax of W C logits and a
        top-W — on the joint logits f[b, t_w] + g_rows[b, w] of the same beam, scores and lengths;
    nabu_transducer_greedy_step.
The beam state is captured mid-search (iteration 60 of a search on seeded N(0, 2) logits with the blank raised by 8.5, so
that a hypothesis emits about 0.3 labels per iteration and none has reached S): every slot is full.  All three update
their state in place, so it is put back before every call, outside the timed interval, and all three are called through
the C ABI on buffers made beforehand.
THE BAR: the beam step takes no longer than 1.5 times the prune launch.  The margin pays for what the step does on
top: the W x W merge test, the copy of S labels per survivor, the finals.
Also, without a bar: the whole search of TransducerDecoder — greedy, W = 4, W = 8 — on the untrained recipe model at
cfg1's size (8 x 200 x 40, max_steps 50), in milliseconds per call of the decoder (encoder included).

Protocol (tools/transducer_bench.py): everything is warmed up; a round times the arms alternately, one call of each per
repetition, between device events, and keeps the median of each; medians of --rounds rounds are reported with the
spread of the rounds ((max - min) / median).

    python tools/transducer_beam_bench.py [--reps 200] [--rounds 5] [--search 5] [--out profiles/transducer_beam.json]

Prints one JSON line and writes it to --out."""
import argparse
import configparser
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = dict(B=32, T=125, C=40, S=50)
WIDTHS = (8, 16)
CAPTURE = 60
MARGIN = 1.5
KEYS = ('ids', 'out_len', 'score', 'parent', 'emit', 'last_id', 'fin_ids', 'fin_len', 'fin_score')


def timed_once(prepare, fn):
    prepare()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rounds_of(arms, reps, rounds, scale=1e3):
    """arms: {name: (prepare, fn)}; medians per round of every arm (alternated) -> (per_round, median, spread)"""
    per_round = {k: [] for k in arms}
    for _ in range(rounds):
        t = {k: [] for k in arms}
        for _ in range(reps):
            for k, (prepare, fn) in arms.items():
                t[k].append(timed_once(prepare, fn))
        for k in arms:
            per_round[k].append(scale * float(np.median(t[k])))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    return ({k: [round(x, 2) for x in v] for k, v in per_round.items()}, {k: round(v, 2) for k, v in med.items()},
            {k: round((max(v) - min(v)) / med[k], 4) for k, v in per_round.items()})


def measure(W, reps, rounds):
    from nabu_amd import _hip, ops
    from nabu_amd._hip import ptr
    dev = torch.device('cuda')
    B, T, C, S = SHAPE['B'], SHAPE['T'], SHAPE['C'], SHAPE['S']
    rng = np.random.default_rng(1000 * T + W)
    fh = (2.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    fh[:, :, C - 1] += 8.5
    f = torch.tensor(fh, device=dev)
    by_last = torch.tensor((1.4 * rng.standard_normal((C, C))).astype(np.float32), device=dev)
    by_len = torch.tensor((1.4 * rng.standard_normal((S + 1, C))).astype(np.float32), device=dev)
    enc_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = ops.transducer_beam_state(B, W, S, dev)

    def g_of():            # prediction logits of a slot from its last label and its length: N(0, 2) as f's
        return (by_last[st.last_id.long()] + by_len[st.out_len.clamp(min=0).long()]).contiguous()
    g_rows = (by_last[C - 1] + by_len[0]).expand(B, W, C).contiguous()
    for it in range(CAPTURE):
        ops.transducer_beam_step(it, f, g_rows, enc_len, st)
        g_rows = g_of()
    assert bool((st.out_len >= 0).all().item()) and int(st.out_len.max().item()) < S, 'the captured beam is not full'
    kept = {k: getattr(st, k).clone() for k in KEYS}
    labels = float(st.out_len.float().mean().item())
    # the prune launch's operands: the joint logits of the same beam
    t_w = (CAPTURE - st.out_len).long()
    joint = (f[torch.arange(B, device=dev)[:, None], t_w] + g_rows).contiguous()
    lp0, len0 = st.score.clone(), st.out_len.clone()
    lp, ln = lp0.clone(), len0.clone()
    zeros = torch.zeros((B, W), dtype=torch.int32, device=dev)
    fin, seen, pred, par, stay = (torch.zeros((B, W), dtype=torch.int32, device=dev) for _ in range(5))
    all_seen = torch.zeros(B, dtype=torch.int32, device=dev)
    scratch = torch.empty((B, W * C + W), dtype=torch.float32, device=dev)
    gs = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(4)]
    g_ids, g_score, g_row = torch.zeros((B, S), dtype=torch.int32, device=dev), torch.zeros(B, device=dev), g_rows[:, 0].contiguous()
    L, s = _hip.lib(), _hip.stream()

    def restore_beam():
        for k in KEYS:
            getattr(st, k).copy_(kept[k])

    def restore_prune():
        lp.copy_(lp0), ln.copy_(len0), fin.copy_(zeros), seen.copy_(zeros)

    def beam():
        _hip.check(L.nabu_transducer_beam_step(B, T, C, S, W, CAPTURE, ptr(f), ptr(g_rows), ptr(enc_len), ptr(st.ids),
                                               ptr(st.out_len), ptr(st.score), ptr(st.parent), ptr(st.emit), ptr(st.last_id),
                                               ptr(st.fin_ids), ptr(st.fin_len), ptr(st.fin_score), ptr(st.ws),
                                               st.ws.numel(), s), 'nabu_transducer_beam_step')

    def prune():
        _hip.check(L.nabu_beam_prune(B, W, C, ptr(joint), 1.0, 0.0, ptr(lp), ptr(ln), ptr(fin), ptr(seen), ptr(pred), ptr(par),
                                     ptr(stay), ptr(all_seen), ptr(scratch), s), 'nabu_beam_prune')

    def greedy():
        _hip.check(L.nabu_transducer_greedy_step(B, T, C, S, 0, ptr(f), ptr(g_row), ptr(enc_len), ptr(gs[0]), ptr(gs[1]),
                                                 ptr(g_ids), ptr(gs[2]), ptr(gs[3]), ptr(g_score), s),
                   'nabu_transducer_greedy_step')
    arms = {'beam_step': (restore_beam, beam), 'prune': (restore_prune, prune), 'greedy_step': (lambda: None, greedy)}
    for _ in range(10):
        for prepare, fn in arms.values():
            prepare()
            fn()
    per_round, med, spread = rounds_of(arms, reps, rounds)
    return {'shape': dict(SHAPE, W=W), 'captured_at': CAPTURE, 'mean_labels_per_slot': round(labels, 2),
            'us_per_round': per_round, 'median_us': med, 'spread': spread,
            'beam_over_prune': round(med['beam_step'] / med['prune'], 4), 'bar': MARGIN,
            'bar_met': bool(med['beam_step'] <= MARGIN * med['prune']),
            'beam_over_greedy': round(med['beam_step'] / med['greedy_step'], 4)}


def measure_search(reps, rounds):
    """TransducerDecoder on the untrained recipe model at cfg1's size: greedy, W = 4, W = 8, ms per call"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.decoders import decoder_factory
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(8, 200, 40, min_frames=200, min_labels=10, max_labels=40, seed=1234)
    mc, tc, ec = recipes.load_recipe('dblstm_transducer_timit')
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=None, task_index=0)
    batch = tr.to_device(data.batch(0))
    alphabet = ' '.join('p%d' % i for i in range(39))
    arms = {}
    for name, width in (('greedy', None), ('beam4', 4), ('beam8', 8)):
        conf = configparser.ConfigParser()
        conf.read_dict({'decoder': dict({'decoder': 'transducer_decoder', 'max_steps': '50', 'text_alphabet': alphabet},
                                        **({'beam_width': str(width)} if width else {}))})
        dec = decoder_factory.factory('transducer_decoder')(conf, tr.model)
        arms[name] = (lambda: None, lambda dec=dec: dec(batch['inputs'], batch['input_seq_length']))
    for _ in range(2):
        for _, fn in arms.values():
            fn()
    per_round, med, spread = rounds_of(arms, reps, rounds, scale=1.0)
    return {'workload': '8 x 200 x 40 fbank, DBLSTM 2 x 256, untrained, max_steps 50', 'ms_per_round': per_round,
            'median_ms': med, 'spread': spread, 'beam4_over_greedy': round(med['beam4'] / med['greedy'], 4),
            'beam8_over_greedy': round(med['beam8'] / med['greedy'], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--search', type=int, default=5, help='searches per round of the whole-search comparison; 0 skips it')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transducer_beam.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'transducer_beam_bench needs a GPU'
    torch.cuda.set_device(0)
    sys.path.insert(0, ROOT)
    res = {'bench': 'transducer_beam', 'reps': args.reps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'cases': [measure(W, args.reps, args.rounds) for W in WIDTHS]}
    if args.search:
        res['search'] = measure_search(args.search, args.rounds)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fid:
        fid.write(line + '\n')


if __name__ == '__main__':
    main()
