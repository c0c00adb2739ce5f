"""GPU tests of the Kaldi-hybrid recipe (DNN encoder, wide cross-entropy, AlignmentDecoder) against float64:
the kernels of nabu_amd/csrc/dnn.hip one by one on ragged lengths, a shrunken recipe's training trajectory, a
full-size step under the shipped arithmetic against exact fp32, and `run decode` end to end."""
import configparser
import os

import numpy as np
import pytest
import torch

from nabu_amd import ops as hip
from nabu_amd import recipes
from nabu_amd.neuralnetworks.components import ops as nops
from nabu_amd.neuralnetworks.models.ed_encoders import dnn as dnn_enc
from nabu_amd.neuralnetworks.trainers import trainer_factory
from nabu_amd.processing.synthetic import SyntheticData
from tests import dnn_ref

pytestmark = pytest.mark.gpu

rel = lambda a, b_: float(np.abs(np.asarray(a, np.float64) - b_).max() / (np.abs(b_).max() + 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- kernels

def test_splice_stack_unstack_stack_bit_exact():
    rng = np.random.default_rng(1)
    B, T, F, c = 5, 23, 13, 3
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    x[3, 15:] = 7.0                                # padding that is not zero: the splice reads it as the reference
    lens = np.array([17, 5, 1, 15, 9], np.int32)  # max(len) = 17 < T
    N, ld = int(lens.sum()), dnn_enc.splice_ld(F, c)
    assert ld == 96 and ld > (2 * c - 1) * F
    S = hip.splice_stack(dev(x), dev(lens), c, N, ld).cpu().numpy()
    ref = dnn_ref.stack_seq(dnn_ref.splice(torch.from_numpy(x), c), lens).numpy()
    assert S.shape == (N, ld)
    assert np.array_equal(S[:, :(2 * c - 1) * F], ref)
    assert np.all(S[:, (2 * c - 1) * F:] == 0)
    for H in (16, 7):                              # float4 and scalar moves
        rows = rng.standard_normal((N, H)).astype(np.float32)
        U = hip.unstack_rows(dev(rows), dev(lens), B, int(lens.max())).cpu().numpy()
        assert U.shape == (B, 17, H)
        assert np.array_equal(U, dnn_ref.unstack_seq(torch.from_numpy(rows), lens).numpy())
        g = rng.standard_normal((B, 17, H)).astype(np.float32)
        R = hip.stack_rows(dev(g), dev(lens), N).cpu().numpy()
        assert np.array_equal(R, dnn_ref.stack_seq(torch.from_numpy(g), lens).numpy())


@pytest.mark.parametrize('F', [2048, 260, 4])
def test_rows_relu_layer_norm_fwd_bwd(F):
    rng = np.random.default_rng(F)
    N = 37
    z = rng.standard_normal((N, F)).astype(np.float32)
    z[3] = -np.abs(z[3]) - 0.1                     # relu kills the row: var 0, rstd = 1/sqrt(eps)
    z[5] = 0.75                                    # constant row
    gamma = (1 + 0.1 * rng.standard_normal(F)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(F)).astype(np.float32)
    dy = rng.standard_normal((N, F)).astype(np.float32)
    y, mean, rstd = hip.rows_relu_ln_fwd(dev(z), dev(gamma), dev(beta))
    dz, dgp, dbp = hip.rows_relu_ln_bwd(dev(z), dev(dy), dev(gamma), mean, rstd)
    dg = torch.zeros(F, device='cuda')
    db = torch.zeros(F, device='cuda')
    hip.colsum(dgp, dg)
    hip.colsum(dbp, db)
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    gt = torch.tensor(gamma.astype(np.float64), requires_grad=True)
    bt = torch.tensor(beta.astype(np.float64), requires_grad=True)
    yt = dnn_ref.relu_layer_norm(zt, gt, bt)
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    assert rel(y.cpu().numpy(), yt.detach().numpy()) <= 1e-5
    assert abs(rstd[3].item() - 1e6) / 1e6 < 1e-6 and np.allclose(y[3].cpu().numpy(), beta)
    assert rel(dz.cpu().numpy(), zt.grad.numpy()) <= 1e-5
    assert np.all(dz[3].cpu().numpy() == 0)
    assert rel(dg.cpu().numpy(), gt.grad.numpy()) <= 1e-5
    assert rel(db.cpu().numpy(), bt.grad.numpy()) <= 1e-5


def test_rows_relu_layer_norm_unsupported_width_falls_back():
    """F % 4 != 0: the kernel says NABU_EUNSUP, the encoder composes relu + layer_norm with the same result"""
    from nabu_amd import variables as vs
    rng = np.random.default_rng(3)
    N, F = 9, 10
    z = rng.standard_normal((N, F)).astype(np.float32)
    assert hip.rows_relu_ln_fwd(dev(z), dev(np.ones(F, np.float32)), dev(np.zeros(F, np.float32))) is None
    with vs.as_default(vs.VariableStore(seed=1)):
        y = dnn_enc._relu_layer_norm(dev(z), 'LN')              # (no tape: nothing is recorded)
    ref = dnn_ref.relu_layer_norm(torch.tensor(z.astype(np.float64)), torch.ones(F, dtype=torch.float64),
                                  torch.zeros(F, dtype=torch.float64))
    assert rel(y.cpu().numpy(), ref.numpy()) <= 1e-5


def _xent_ref(logits, targets, lens, tlens):
    lg = torch.tensor(logits.astype(np.float64), requires_grad=True)
    B, L, C = logits.shape
    logp = torch.log_softmax(lg, -1)
    nll = -logp.gather(2, torch.tensor(targets[:, :L].astype(np.int64))[:, :, None])[:, :, 0]
    mask = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    per = (nll * mask).sum(1) / torch.tensor(tlens.astype(np.float64))
    per.sum().backward()
    return per.detach().numpy(), lg.grad.numpy()


@pytest.mark.parametrize('C', [1024, 1031, 3100, 4099])
def test_wide_cross_entropy(C):
    rng = np.random.default_rng(C)
    B, L = 5, 19
    logits = (3 * rng.standard_normal((B, L, C))).astype(np.float32)
    lens = np.array([19, 4, 11, 1, 16], np.int32)
    targets = rng.integers(0, C, (B, L + 2)).astype(np.int32)
    tlens = np.array([19, 4, 11, 1, 16], np.int32)
    scale = 0.2
    loss, dl = hip.xent_wide_loss_grad(dev(logits), dev(targets), dev(lens), dev(tlens), scale)
    per, g = _xent_ref(logits, targets, lens, tlens)
    assert rel(loss.cpu().numpy(), per) <= 1e-6
    assert rel(dl.cpu().numpy(), scale * g) <= 1e-5
    assert np.all(dl.cpu().numpy()[1, 4:] == 0)
    loss2, dl2 = hip.xent_wide_loss_grad(dev(logits), dev(targets), dev(lens), dev(tlens), scale)
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2)                    # deterministic
    if C == 1024:                                  # the routing threshold: both kernels agree
        l0, d0 = hip.xent_loss_grad(dev(logits), dev(targets), dev(lens), dev(tlens), scale)
        assert rel(loss.cpu().numpy(), l0.cpu().numpy().astype(np.float64)) <= 1e-6
        assert rel(dl.cpu().numpy(), d0.cpu().numpy().astype(np.float64)) <= 1e-5
    # an unaligned view (rows off their 16-byte phase) takes the scalar head / tail
    buf = torch.zeros(B * L * C + 1, device='cuda')
    v = buf[1:].view(B, L, C)
    v.copy_(dev(logits))
    l3, d3 = hip.xent_wide_loss_grad(v, dev(targets), dev(lens), dev(tlens), scale)
    assert rel(l3.cpu().numpy(), per) <= 1e-6 and rel(d3.cpu().numpy(), scale * g) <= 1e-5


def test_loss_routing_threshold():
    from nabu_amd.neuralnetworks.trainers import loss_functions as lf
    assert lf.WIDE_XENT_MIN_CLASSES == 1024


@pytest.mark.parametrize('C', [1031, 3100])
def test_log_softmax_prior(C):
    rng = np.random.default_rng(C + 1)
    B, T = 3, 9
    x = (2 * rng.standard_normal((B, T, C))).astype(np.float32)
    lens = np.array([9, 2, 5], np.int32)
    prior = rng.random(C) + 0.1
    prior /= prior.sum()
    for lp in (np.log(prior), np.log(np.ones(C) / C)):
        out = hip.log_softmax_prior(dev(x), dev(lens), dev(lp.astype(np.float32))).cpu().numpy()
        ref = torch.log_softmax(torch.tensor(x.astype(np.float64)), -1).numpy() - lp
        for b in range(B):
            assert rel(out[b, :lens[b]], ref[b, :lens[b]]) <= 1e-6
            assert np.all(out[b, lens[b]:] == 0)


# ------------------------------------------------------------------------------------------------- model level

def _trainer(data, **over):
    mc, tc, ec = recipes.load_recipe('dnn_hybrid_wsj', **over)
    return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                               server=None, task_index=0)


SMALL = {'encoder.context': 3, 'encoder.num_units': 256, 'encoder.num_layers': 3, 'encoder.dropout': 0.8,
         'encoder.gemm_precision': 'f32', 'io.output_dims': 1031, 'trainer.batch_size': 6}


def test_shrunken_recipe_trajectory_matches_float64():
    from oracle import nabu_oracle as O
    data = SyntheticData(6, 40, 13, num_labels=1031, min_frames=12, frame_targets=True, target_name='alignments',
                         seed=77)
    nops.set_seed(91)
    tr = _trainer(data, **SMALL)
    b0 = tr.to_device(data.batch(0))
    with torch.no_grad():
        tr.model(b0['inputs'], b0['input_seq_length'], b0['targets'], b0['target_seq_length'], False)
    keys = dnn_ref.names('features', 'alignments', 3)
    st = tr.model.store.state_dict()
    params = {k: st[k].astype(np.float64) for k in keys}
    ms = {k: np.zeros_like(v) for k, v in params.items()}
    vs_ = {k: np.zeros_like(v) for k, v in params.items()}
    losses, ref = [], []
    for s in range(20):
        raw = data.batch(s)
        lens = raw['input_seq_length']['features']
        rng = nops.global_rng()
        masks = dnn_ref.dropout_masks(int(lens.sum()), 256, 3, 0.8, rng.seed, rng.offset)
        loss = tr.step(tr.to_device(raw))
        lr = tr.learning_rate()                    # (constant within train-free steps: global_step stays 0)
        losses.append(float(loss.item()))
        l64, g64 = dnn_ref.step(params, raw['inputs']['features'], lens, raw['targets']['alignments'],
                                raw['target_seq_length']['alignments'], 3, 3, masks=masks)
        ref.append(l64)
        if s == 0:
            got = {k: v.grad.cpu().numpy() for k, v in tr.model.store.vars.items() if k in keys}
            for k in keys:
                assert rel(got[k], g64[k]) <= 1e-4, (k, rel(got[k], g64[k]))
        for k in keys:
            params[k], ms[k], vs_[k] = O.clip_adam_update(params[k], g64[k], ms[k], vs_[k], s + 1, lr)
    r = np.abs(np.array(losses) - ref) / np.abs(ref)
    assert r.max() <= 1e-4, (losses, ref)


def test_full_size_step_shipped_arithmetic_against_f32():
    B, T = 32, 1000
    data = SyntheticData(B, T, 123, num_labels=3100, min_frames=500, frame_targets=True, target_name='alignments',
                         seed=5)
    raw = data.batch(0)
    out = {}
    mc, _, _ = recipes.load_recipe('dnn_hybrid_wsj')
    shipped = mc.get('encoder', 'gemm_precision')
    for prec in (shipped, 'f32'):
        tr = _trainer(data, **{'encoder.gemm_precision': prec})
        from nabu_amd.autodiff import Tape
        from nabu_amd.neuralnetworks.trainers import loss_functions
        batch = tr.to_device(raw)
        with Tape() as tape:
            logits, lsl = tr.model(batch['inputs'], batch['input_seq_length'], batch['targets'],
                                   batch['target_seq_length'], True)
            loss = loss_functions.average_cross_entropy(batch['targets'], logits, lsl, batch['target_seq_length'])
        tape.backward(loss)
        out[prec] = (float(loss.item()), {k: v.grad.cpu().numpy().astype(np.float64)
                                          for k, v in tr.model.store.vars.items()})
        del tr, tape, logits, loss, batch
    (la, ga), (lb, gb) = out[shipped], out['f32']
    assert abs(la - lb) / abs(lb) <= 1e-4, (la, lb)
    assert set(ga) == set(gb) and len(ga) == 5 * 4 + 2
    for k in gb:
        assert rel(ga[k], gb[k]) <= 1e-3, (k, rel(ga[k], gb[k]))


def test_run_decode_writes_loglikes(tmp_path, capsys):
    """train-free decode of a small feature set through scripts.decode -> Recognizer -> AlignmentDecoder: the ark
    holds log_softmax(logits) - log(prior) of every utterance, cut to its length"""
    from nabu_amd.processing.tfwriters.array_writer import ArrayWriter
    from nabu_amd.scripts import decode as run_decode
    from nabu_amd.scripts.test import load_model
    from tests.test_dnn_recipe import read_ark
    rng = np.random.default_rng(8)
    F, C = 13, 1031
    feats_dir = tmp_path / 'feats'
    w = ArrayWriter(str(feats_dir))
    lens = [14, 6, 9]
    feats = []
    for i, n in enumerate(lens):
        f = rng.standard_normal((n, F)).astype(np.float32)
        feats.append(f)
        w.write(f, 'utt%d' % i)
    (feats_dir / 'max_length').write_text(str(max(lens)))
    hist = np.zeros(max(lens) + 1)
    for n in lens:
        hist[n] += 1
    np.save(str(feats_dir / 'sequence_length_histogram.npy'), hist)
    (feats_dir / 'dim').write_text(str(F))
    expdir = tmp_path / 'exp'
    expdir.mkdir()
    mc, _, _ = recipes.load_recipe('dnn_hybrid_wsj', **{'encoder.context': 2, 'encoder.num_units': 64,
                                                         'encoder.num_layers': 2, 'io.output_dims': C})
    with open(expdir / 'model.cfg', 'w') as fid:
        mc.write(fid)
    prior = rng.random(C) + 0.05
    prior /= prior.sum()
    np.save(str(tmp_path / 'prior.npy'), prior)
    db = configparser.ConfigParser()
    db.read_dict({'testfbank': {'type': 'audio_feature', 'dir': str(feats_dir), 'datafiles': 'none'}})
    with open(expdir / 'database.conf', 'w') as fid:
        db.write(fid)
    rc = configparser.ConfigParser()
    rc.read_dict({'recognizer': {'batch_size': '2', 'features': 'testfbank'},
                  'decoder': {'decoder': 'alignment_decoder', 'prior': str(tmp_path / 'prior.npy')}})
    with open(expdir / 'recognizer.cfg', 'w') as fid:
        rc.write(fid)
    tc = configparser.ConfigParser()
    tc.read_dict({'trainer': {'trainlabels': '0'}})
    with open(expdir / 'trainer.cfg', 'w') as fid:
        tc.write(fid)
    # the weights decode reads: this model's, after a first call created them
    from nabu_amd.autodiff import SeqLen
    model = load_model(str(expdir), False)
    with torch.no_grad():
        model({'features': dev(feats[0][None])}, {'features': SeqLen([lens[0]])}, [], [], False)
    (expdir / 'model').mkdir()
    np.savez(str(expdir / 'model' / 'network.ckpt.npz'), **model.store.state_dict())
    directory = run_decode.decode(str(expdir))
    mats = read_ark(os.path.join(directory, 'alignments', 'feats.scp'))
    assert sorted(mats) == ['utt0', 'utt1', 'utt2']
    with torch.no_grad():
        for i, n in enumerate(lens):
            lg, _ = model({'features': dev(feats[i][None])}, {'features': SeqLen([n])}, [], [], False)
            l64 = lg['alignments'][0].cpu().numpy().astype(np.float64)
            ref = torch.log_softmax(torch.from_numpy(l64), -1).numpy() - np.log(prior)
            got = mats['utt%d' % i]
            assert got.shape == (n, C)
            assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
