"""Float64 restatement of the Speller over M encoded inputs (one attention mechanism each): TF-1.8 AttentionWrapper
with a list of mechanisms, attention_layer_size=None, output_attention=False, as the reference builds it at
nabu/neuralnetworks/models/ed_decoders/speller.py:49-61 [TF-1.8 recalled for the wrapper's wiring].

  cell input of step t   [onehot(y_{t-1}) | ctx_0(t-1) | .. | ctx_{M-1}(t-1)]
  per mechanism m        q_m = h_top . Wq_m;  align_m, ctx_m exactly as the one-memory oracle (oracle/nabu_oracle.py)
  logits                 [h_top | ctx_0(t) | .. | ctx_{M-1}(t)] . Wout + b

NumPy forward and analytic backward (multi_speller_fwd / multi_speller_bwd), built on the oracle's attention pieces,
and an independent PyTorch-CPU autograd statement (torch_multi_speller) in the style of tests/torch_ref.py.

Parameters: dict(lstm=[dict(kernel, bias)], mem=[dict(memory_kernel, query_kernel, attention_v[, conv_kernel,
conv_proj]) per memory], out_kernel [(U + sum E), C], out_bias [C]); lstm[0].kernel [(C + sum E + U), 4U]."""
import numpy as np

from oracle import nabu_oracle as O


def from_single(p):
    """the one-memory oracle's parameter dict in this file's form"""
    mem = {k: p[k] for k in ('memory_kernel', 'query_kernel', 'attention_v', 'conv_kernel', 'conv_proj') if k in p}
    return dict(lstm=p['lstm'], mem=[mem], out_kernel=p['out_kernel'], out_bias=p['out_bias'])


def multi_speller_fwd(encs, enc_lens, targets, target_len, p, attention='vanilla', probability_fn='softmax',
                      dec_inputs=None, window=None, out_masks=None):
    """encs: list of [B,Te_m,E_m]; enc_lens: list of [B].  Returns logits [B,L,C], target_len, cache."""
    M = len(encs)
    B = encs[0].shape[0]
    dt = encs[0].dtype
    C = p['out_bias'].shape[0]
    U = p['mem'][0]['attention_v'].shape[0]
    target_len = np.asarray(target_len)
    L = int(target_len.max())
    masks = [np.arange(e.shape[1])[None, :] < np.asarray(l)[:, None] for e, l in zip(encs, enc_lens)]
    values = [e * m[:, :, None] for e, m in zip(encs, masks)]
    keys = [v @ pm['memory_kernel'] for v, pm in zip(values, p['mem'])]
    nl = len(p['lstm'])
    hs = [np.zeros((B, U), dt) for _ in range(nl)]
    cs = [np.zeros((B, U), dt) for _ in range(nl)]
    ctx = [np.zeros((B, e.shape[2]), dt) for e in encs]
    align = [np.zeros((B, e.shape[1]), dt) for e in encs]
    if attention == 'windowed':
        for a in align:
            a[:, 0] = 1
    inp_ids = np.concatenate([np.full((B, 1), C - 1, np.int64), np.asarray(targets)[:, :L].astype(np.int64)], 1)
    if dec_inputs is not None:
        inp_ids = np.asarray(dec_inputs).astype(np.int64)
    logits = np.zeros((B, L, C), dt)
    steps = []
    for t in range(L):
        act = (t < target_len)[:, None]
        onehot = np.zeros((B, C), dt)
        onehot[np.arange(B), inp_ids[:, t]] = 1
        x = np.concatenate([onehot] + ctx, 1)
        st = dict(act=act, cs_prev=[c.copy() for c in cs], align_prev=list(align), lstm=[], mem=[])
        nh, nc = [], []
        for n in range(nl):
            xin = np.concatenate([x, hs[n]], 1)
            z = xin @ p['lstm'][n]['kernel'] + p['lstm'][n]['bias']
            i = O.sigmoid(z[:, :U]); g = np.tanh(z[:, U:2 * U])
            f = O.sigmoid(z[:, 2 * U:3 * U] + O.FORGET_BIAS); o = O.sigmoid(z[:, 3 * U:])
            c = cs[n] * f + i * g
            h = np.tanh(c) * o
            st['lstm'].append(dict(xin=xin, i=i, g=g, f=f, o=o, c=c))
            nh.append(h); nc.append(c)
            x = h if out_masks is None else h * out_masks[t][n]
        query = x
        cxs, als = [], []
        for m in range(M):
            pm = p['mem'][m]
            s = keys[m] + (query @ pm['query_kernel'])[:, None, :]
            sm = {}
            pmask = masks[m]
            if attention == 'location_aware':
                sm['cf'] = O.conv1d_same(align[m], pm['conv_kernel'])
                s = s + sm['cf'] @ pm['conv_proj']
            elif attention == 'windowed':
                pmask = masks[m] & O.attention_window(align[m], window[0], window[1])
            elif attention != 'vanilla':
                raise ValueError(attention)
            th = np.tanh(s)
            score = th @ pm['attention_v']
            al = O._prob_fwd(score, pmask, probability_fn)
            cx = np.einsum('bt,bte->be', al, values[m])
            sm.update(th=th, score=score, al=al, cx=cx, pmask=pmask)
            st['mem'].append(sm)
            cxs.append(cx); als.append(al)
        lg = np.concatenate([query] + cxs, 1) @ p['out_kernel'] + p['out_bias']
        st['query'] = query
        steps.append(st)
        logits[:, t] = np.where(act, lg, 0)
        hs = [np.where(act, a, b_) for a, b_ in zip(nh, hs)]
        cs = [np.where(act, a, b_) for a, b_ in zip(nc, cs)]
        ctx = [np.where(act, a, b_) for a, b_ in zip(cxs, ctx)]
        align = [np.where(act, a, b_) for a, b_ in zip(als, align)]
    cache = dict(steps=steps, p=p, values=values, keys=keys, masks=masks, attention=attention,
                 probability_fn=probability_fn, U=U, C=C, out_masks=out_masks)
    return logits, target_len.copy(), cache


def multi_speller_bwd(dlogits, cache):
    """Gradient of multi_speller_fwd: returns [d enc_m] and the parameter gradients (same structure as p)."""
    p, steps = cache['p'], cache['steps']
    values, keys, masks = cache['values'], cache['keys'], cache['masks']
    att, pf, U, C = cache['attention'], cache['probability_fn'], cache['U'], cache['C']
    om = cache.get('out_masks')
    M = len(values)
    B = values[0].shape[0]
    dt = values[0].dtype
    Es = [v.shape[2] for v in values]
    off = np.concatenate([[0], np.cumsum(Es)]).astype(int)
    nl = len(p['lstm'])
    g = dict(out_kernel=np.zeros_like(p['out_kernel']), out_bias=np.zeros_like(p['out_bias']),
             lstm=[dict(kernel=np.zeros_like(q['kernel']), bias=np.zeros_like(q['bias'])) for q in p['lstm']],
             mem=[{k: np.zeros_like(v) for k, v in pm.items()} for pm in p['mem']])
    dvalues = [np.zeros_like(v) for v in values]
    dkeys = [np.zeros_like(k) for k in keys]
    dhs = [np.zeros((B, U), dt) for _ in range(nl)]
    dcs = [np.zeros((B, U), dt) for _ in range(nl)]
    dctx = [np.zeros((B, E), dt) for E in Es]
    dalign = [np.zeros((B, v.shape[1]), dt) for v in values]
    for t in range(len(steps) - 1, -1, -1):
        st = steps[t]
        act = st['act']
        dl = np.where(act, dlogits[:, t], 0)
        qc = np.concatenate([st['query']] + [sm['cx'] for sm in st['mem']], 1)
        g['out_kernel'] += qc.T @ dl
        g['out_bias'] += dl.sum(0)
        dqc = dl @ p['out_kernel'].T
        dx = dqc[:, :U].copy()
        ndalign = []
        for m in range(M):
            sm, pm, gm = st['mem'][m], p['mem'][m], g['mem'][m]
            dcx = dqc[:, U + off[m]:U + off[m + 1]] + np.where(act, dctx[m], 0)
            dal = np.einsum('be,bte->bt', dcx, values[m]) + np.where(act, dalign[m], 0)
            dvalues[m] += sm['al'][:, :, None] * dcx[:, None, :]
            dscore = np.where(act, O._prob_bwd(dal, sm['al'], sm['score'], sm['pmask'], pf), 0)
            gm['attention_v'] += np.einsum('bt,btu->u', dscore, sm['th'])
            ds = dscore[:, :, None] * pm['attention_v'] * (1 - sm['th'] ** 2)
            dkeys[m] += ds
            dq = ds.sum(1)
            dalign_prev = np.zeros_like(dalign[m])
            if att == 'location_aware':
                gm['conv_proj'] += np.einsum('btf,btu->fu', sm['cf'], ds)
                dalign_prev, dck = O.conv1d_same_bwd(ds @ pm['conv_proj'].T, st['align_prev'][m], pm['conv_kernel'])
                gm['conv_kernel'] += dck
            gm['query_kernel'] += st['query'].T @ dq
            dx += dq @ pm['query_kernel'].T
            ndalign.append(np.where(act, dalign_prev, dalign[m]))
        ndhs, ndcs = [None] * nl, [None] * nl
        for n in range(nl - 1, -1, -1):
            c_ = st['lstm'][n]
            i, gg, f, o, c = c_['i'], c_['g'], c_['f'], c_['o'], c_['c']
            tc = np.tanh(c)
            if om is not None:
                dx = dx * om[t][n]
            dh = np.where(act, dx + dhs[n], 0)
            dc = np.where(act, dcs[n], 0) + dh * o * (1 - tc * tc)
            dz = np.concatenate([dc * gg * i * (1 - i), dc * i * (1 - gg * gg), dc * st['cs_prev'][n] * f * (1 - f),
                                 dh * tc * o * (1 - o)], 1)
            g['lstm'][n]['kernel'] += c_['xin'].T @ dz
            g['lstm'][n]['bias'] += dz.sum(0)
            dxin = dz @ p['lstm'][n]['kernel'].T
            nin = c_['xin'].shape[1] - U
            ndhs[n] = np.where(act, dxin[:, nin:], dhs[n])
            ndcs[n] = np.where(act, dc * f, dcs[n])
            dx = dxin[:, :nin]
        dhs, dcs = ndhs, ndcs
        dctx = [np.where(act, dx[:, C + off[m]:C + off[m + 1]], dctx[m]) for m in range(M)]
        dalign = ndalign
    for m in range(M):
        g['mem'][m]['memory_kernel'] += values[m].reshape(-1, Es[m]).T @ dkeys[m].reshape(-1, U)
        dvalues[m] += dkeys[m] @ p['mem'][m]['memory_kernel'].T
        dvalues[m] *= masks[m][:, :, None]
    return dvalues, g


def make_params(rng, C, U, Es, nl, attention='vanilla', K=3, F=2, scale=0.4):
    """random float64 parameters of an M-memory speller"""
    SE = sum(Es)
    r = lambda *s: rng.uniform(-scale, scale, s)
    p = dict(lstm=[dict(kernel=r((C + SE if n == 0 else U) + U, 4 * U), bias=r(4 * U)) for n in range(nl)],
             out_kernel=r(U + SE, C), out_bias=r(C), mem=[])
    for E in Es:
        pm = dict(memory_kernel=r(E, U), query_kernel=r(U, U), attention_v=r(U))
        if attention == 'location_aware':
            pm.update(conv_kernel=r(K, F), conv_proj=r(F, U))
        p['mem'].append(pm)
    return p


def flat_items(p):
    """[(name, array)] over every parameter array of p (the arrays themselves, not copies)"""
    out = [('out_kernel', p['out_kernel']), ('out_bias', p['out_bias'])]
    for n, q in enumerate(p['lstm']):
        out += [('lstm%d/kernel' % n, q['kernel']), ('lstm%d/bias' % n, q['bias'])]
    for m, pm in enumerate(p['mem']):
        out += [('mem%d/%s' % (m, k), v) for k, v in sorted(pm.items())]
    return out


def brute_force_beam_search(encs, enc_lens, p, beam_width, max_steps, attention='vanilla', probability_fn='softmax',
                            window=None):
    """Beam search (components/beam_search_decoder.py semantics as oracle/decode_oracle.py restates them, length
    penalty 0, temperature 1) by enumeration: a hypothesis is its label prefix, and the log-probabilities of its
    continuations come from running multi_speller_fwd over the WHOLE prefix again — no state is carried, pruned or
    gathered, so a wrong gather of any of the M alignment states or of the contexts cannot be reproduced here.
    Returns per utterance a list of W (labels tuple, length, logprob, alignments per memory [time, Te_m]) best first,
    the smallest gap between neighbouring candidate scores around the kept ones over all steps, and the step count."""
    B = encs[0].shape[0]
    C = p['out_bias'].shape[0]
    end, W = C - 1, int(beam_width)
    hist = []                                            # per utterance: per step (beams, all slots seen, gap)
    for b in range(B):
        e1 = [e[b:b + 1] for e in encs]
        l1 = [np.asarray(l)[b:b + 1] for l in enc_lens]

        def step_logprobs(prefix):
            n = len(prefix) + 1
            di = np.array([[end] + list(prefix)])
            lg, _, cache = multi_speller_fwd(e1, l1, np.zeros((1, n), int), [n], p, attention, probability_fn,
                                             dec_inputs=di, window=window)
            x = lg[0, n - 1]
            return x - (x.max() + np.log(np.exp(x - x.max()).sum())), [[st['mem'][m]['al'][0] for st in cache['steps']]
                                                                        for m in range(len(encs))]
        beams = [((), (), 0, 0.0, False, [[] for _ in encs])]     # emitted labels, live prefix, length, logprob, finished, aligns
        seen_slots = [False] * W                 # dynamic_decode's stop test is per beam SLOT: finished at some step
        steps = []
        for t in range(int(max_steps)):
            cand = []
            for i, (lab, live, ln, lp, fin, al) in enumerate(beams):
                if fin:                          # "stay": behind all expansions in the candidate order
                    cand.append((lp, W * C + i, lab + (end,), live, ln, True, al))
                    continue
                lps, als = step_logprobs(live)
                for c in range(C):
                    cand.append((lp + lps[c], i * C + c, lab + (c,), live + (c,), ln + (c != end), c == end, als))
            cand.sort(key=lambda x: (-x[0], x[1]))
            sc = [x[0] for x in cand]
            g = min([sc[k] - sc[k + 1] for k in range(min(W, len(sc) - 1))] + [np.inf])
            beams = [(lab, live, ln, lp, fin, al) for lp, _, lab, live, ln, fin, al in cand[:W]]
            seen_slots = [a or x[4] for a, x in zip(seen_slots, beams)]
            steps.append((beams, all(seen_slots) and len(beams) == W, g))
        hist.append(steps)
    # the loop stops for the whole batch at the first step after which every slot of every utterance has been finished
    T = next((t + 1 for t in range(int(max_steps)) if all(h[t][1] for h in hist)), int(max_steps))
    gap = min(h[t][2] for h in hist for t in range(T))
    out = [[(lab, ln, lp, fin, None, al) for lab, live, ln, lp, fin, al in h[T - 1][0]] for h in hist]
    return out, gap, T


# --------------------------------------------------------------------------
# independent statement: PyTorch CPU float64, gradients by autograd
def torch_multi_speller(encs, enc_lens, targets, target_len, p, attention='vanilla', probability_fn='softmax',
                        window=None):
    """Returns (logits tensor [B,L,C], leaves) — leaves: dict(enc=[...], and the parameters by flat_items name), all
    requiring grad.  Written from the semantics in the module docstring with torch primitives only (F.conv1d,
    torch.softmax, torch.where), not from the NumPy code above."""
    import torch
    import torch.nn.functional as Fn
    td = torch.float64
    M = len(encs)
    leaves = {n: torch.tensor(np.asarray(a), dtype=td, requires_grad=True) for n, a in flat_items(p)}
    enc_t = [torch.tensor(np.asarray(e), dtype=td, requires_grad=True) for e in encs]
    leaves['enc'] = enc_t
    B = encs[0].shape[0]
    C = p['out_bias'].shape[0]
    U = p['mem'][0]['attention_v'].shape[0]
    nl = len(p['lstm'])
    tl = torch.tensor(np.asarray(target_len))
    L = int(tl.max())
    valid = [torch.arange(e.shape[1])[None, :] < torch.tensor(np.asarray(l))[:, None] for e, l in zip(encs, enc_lens)]
    vals = [e * v[:, :, None].to(td) for e, v in zip(enc_t, valid)]
    keys = [v @ leaves['mem%d/memory_kernel' % m] for m, v in enumerate(vals)]
    h = [torch.zeros(B, U, dtype=td) for _ in range(nl)]
    c = [torch.zeros(B, U, dtype=td) for _ in range(nl)]
    ctx = [torch.zeros(B, e.shape[2], dtype=td) for e in encs]
    al = [torch.zeros(B, e.shape[1], dtype=td) for e in encs]
    if attention == 'windowed':
        al = [torch.cat([torch.ones(B, 1, dtype=td), a[:, 1:]], 1) for a in al]
    ids = torch.cat([torch.full((B, 1), C - 1, dtype=torch.long), torch.tensor(np.asarray(targets))[:, :L].long()], 1)
    outs = []
    for t in range(L):
        act = (t < tl)[:, None]
        x = torch.cat([Fn.one_hot(ids[:, t], C).to(td)] + ctx, 1)
        nh, ncs = [], []
        for n in range(nl):
            z = torch.cat([x, h[n]], 1) @ leaves['lstm%d/kernel' % n] + leaves['lstm%d/bias' % n]
            zi, zj, zf, zo = z.split(U, 1)
            cn = c[n] * torch.sigmoid(zf + 1.0) + torch.sigmoid(zi) * torch.tanh(zj)
            hn = torch.tanh(cn) * torch.sigmoid(zo)
            nh.append(hn); ncs.append(cn)
            x = hn
        nctx, nal = [], []
        for m in range(M):
            pre = 'mem%d/' % m
            s = keys[m] + (x @ leaves[pre + 'query_kernel'])[:, None, :]
            ok = valid[m]
            if attention == 'location_aware':
                ck = leaves[pre + 'conv_kernel']                       # [K,F]
                K = ck.shape[0]
                pb = (K - 1) // 2
                sig = Fn.pad(al[m][:, None, :], (pb, K - 1 - pb))      # 'same' padding of tf.layers.conv1d
                cf = Fn.conv1d(sig, ck.t()[:, None, :]).transpose(1, 2)   # [B,Te,F]
                s = s + cf @ leaves[pre + 'conv_proj']
            elif attention == 'windowed':
                Te = al[m].shape[1]
                over = torch.cumsum(al[m], 1) > 0.5
                first = torch.where(over.any(1), over.to(torch.int64).argmax(1), torch.full((B,), Te))
                pos = torch.arange(Te)[None, :]
                ok = ok & (pos >= (first[:, None] - window[0] - 1)) & (pos < (first[:, None] + window[1]))
            score = torch.tanh(s) @ leaves[pre + 'attention_v']
            if probability_fn == 'softmax':
                a = torch.softmax(score.masked_fill(~ok, float('-inf')), 1)
            else:
                a = torch.sigmoid(score) * ok.to(td)
                if probability_fn == 'normalized_sigmoid':
                    a = a / a.sum(1, keepdim=True)
            nal.append(a)
            nctx.append(torch.einsum('bt,bte->be', a, vals[m]))
        lg = torch.cat([x] + nctx, 1) @ leaves['out_kernel'] + leaves['out_bias']
        outs.append(torch.where(act, lg, torch.zeros_like(lg)))
        h = [torch.where(act, a, b_) for a, b_ in zip(nh, h)]
        c = [torch.where(act, a, b_) for a, b_ in zip(ncs, c)]
        ctx = [torch.where(act, a, b_) for a, b_ in zip(nctx, ctx)]
        al = [torch.where(act, a, b_) for a, b_ in zip(nal, al)]
    return torch.stack(outs, 1), leaves
