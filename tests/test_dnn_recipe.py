"""CPU tests of the Kaldi-hybrid recipe's host side (no kernel launches): the reference's DNN/WSJ cfgs and
config/recipes/dnn_hybrid_wsj build a trainer, the factories resolve dnn / alignment / alignment_decoder, the
alignment data round trip, the frame-target synthetic batches, the Kaldi ark writer, the splice order."""
import os
import struct

import numpy as np
import pytest
import torch

from nabu_amd import recipes

REF = '/root/reference'


def read_ark(scp_file):
    '''{name: float32 [rows, cols]} of the matrices a feats.scp points at (offset = the NUL after the key)'''
    out = {}
    with open(scp_file) as fid:
        for line in fid:
            name, loc = line.split()
            path, off = loc.rsplit(':', 1)
            with open(path, 'rb') as ark:
                ark.seek(int(off))
                assert ark.read(5) == b'\0BFM '
                size, rows = struct.unpack('<bi', ark.read(5))
                assert size == 4
                size, cols = struct.unpack('<bi', ark.read(5))
                assert size == 4
                out[name] = np.frombuffer(ark.read(4 * rows * cols), '<f4').reshape(rows, cols)
    return out


def _check_dnn_trainer(mc, tc):
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(4, 32, 123, num_labels=3100, frame_targets=True, target_name='alignments',
                         batches_per_epoch=3)
    ec = recipes.from_dict({'evaluator': {'evaluator': 'None'}})
    tr = trainer_factory.factory(tc.get('trainer', 'trainer'))(
        conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None, server=None, task_index=0)
    enc = tr.model.encoder.conf
    assert type(tr.model.encoder).__name__ == 'DNN'
    assert (enc['num_units'], enc['num_layers'], enc['context'], enc['layer_norm']) == ('2048', '5', '5', 'True')
    assert tr.model.output_dims == {'alignments': 3100}
    assert tr.conf['loss'] == 'average_cross_entropy'
    assert tr.model.decoder.conf['num_layers'] == '0'
    assert tr.train(testing=True) == []
    return tr


@pytest.mark.skipif(not os.path.isdir(REF), reason='reference not mounted')
def test_reference_dnn_wsj_cfgs_load_unmodified():
    d = os.path.join(REF, 'config', 'recipes', 'DNN', 'WSJ')
    tr = _check_dnn_trainer(recipes.read_cfg(os.path.join(d, 'model.cfg')),
                            recipes.read_cfg(os.path.join(d, 'trainer.cfg')))
    assert tr.model.encoder.conf['gemm_precision'] == 'default'          # the build addition's default


def test_dnn_hybrid_wsj_recipe_constructs():
    mc, tc, ec = recipes.load_recipe('dnn_hybrid_wsj')
    tr = _check_dnn_trainer(mc, tc)
    assert tr.conf['batch_size'] == '32' and tr.model.encoder.conf['dropout'] == '1'
    assert ec.get('evaluator', 'loss') == 'average_cross_entropy'


def test_synthetic_section_takes_names():
    """a database.conf [synthetic] section may name the targets (trainer.py: non-numeric values stay strings)"""
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe('dnn_hybrid_wsj', **{'encoder.num_units': 16, 'encoder.num_layers': 1})
    dataconf = recipes.from_dict({'synthetic': {'max_frames': 20, 'feature_dim': 123, 'num_labels': 3100,
                                                'frame_targets': True, 'target_name': 'alignments'}})
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=dataconf, modelconf=mc, evaluatorconf=ec,
                                             expdir=None, server=None, task_index=0)
    data = tr._data()
    assert data.target_name == 'alignments' and data.frame_targets is True and data.B == 32


def test_factories_resolve_the_hybrid_names():
    from nabu_amd.neuralnetworks.models.ed_encoders import ed_encoder_factory, dnn
    from nabu_amd.processing.tfreaders import tfreader_factory, alignment_reader
    from nabu_amd.processing.tfwriters import tfwriter_factory, alignment_writer
    from nabu_amd.neuralnetworks.decoders import decoder_factory, alignment_decoder
    assert ed_encoder_factory.factory('dnn') is dnn.DNN
    assert tfreader_factory.factory('alignment') is alignment_reader.AlignmentReader
    assert tfwriter_factory.factory('alignment') is alignment_writer.AlignmentWriter
    assert decoder_factory.factory('alignment_decoder') is alignment_decoder.AlignmentDecoder
    for fac, name in [(tfreader_factory.factory, 'binary'), (tfwriter_factory.factory, 'binary'),
                      (decoder_factory.factory, 'max_decoder'), (ed_encoder_factory.factory, 'hotstart_encoder')]:
        with pytest.raises(Exception, match='outside the MI355X hot path'):
            fac(name)


def test_alignment_round_trip_through_record_data(tmp_path):
    from nabu_amd.processing.tfwriters.alignment_writer import AlignmentWriter
    from nabu_amd.processing.tfwriters.array_writer import ArrayWriter
    from nabu_amd.processing.input_pipeline import RecordData
    rng = np.random.default_rng(4)
    lens = [7, 3, 12, 5]
    fw, aw = ArrayWriter(str(tmp_path / 'f')), AlignmentWriter(str(tmp_path / 'a'))
    feats, alis = [], []
    for i, n in enumerate(lens):
        f = rng.standard_normal((n, 6)).astype(np.float32)
        a = rng.integers(0, 3100, n).astype(np.int32)
        fw.write(f, 'utt%d' % i)
        aw.write(a, 'utt%d' % i)
        feats.append(f)
        alis.append(a)
    (tmp_path / 'f' / 'max_length').write_text(str(max(lens)))
    hist = np.zeros(max(lens) + 1)
    for n in lens:
        hist[n] += 1
    np.save(str(tmp_path / 'f' / 'sequence_length_histogram.npy'), hist)
    (tmp_path / 'f' / 'dim').write_text('6')
    assert (tmp_path / 'a' / 'max_length').read_text() == '12'
    assert np.array_equal(np.load(str(tmp_path / 'a' / 'sequence_length_histogram.npy')), hist)
    assert int((tmp_path / 'a' / 'dim').read_text()) == max(int(a.max()) for a in alis) + 1
    data = RecordData(['features'], [[{'type': 'audio_feature', 'dir': str(tmp_path / 'f')}]],
                      ['alignments'], [[{'type': 'alignment', 'dir': str(tmp_path / 'a')}]], batch_size=4,
                      shuffle=False)
    b = data.batch(0)
    data.close()
    n = b['input_seq_length']['features']
    assert list(n) == lens and list(b['target_seq_length']['alignments']) == lens
    y = b['targets']['alignments']
    assert y.dtype == np.int32 and y.shape == (4, 12)
    for i in range(4):
        assert np.array_equal(y[i, :lens[i]], alis[i]) and np.all(y[i, lens[i]:] == 0)
        assert np.array_equal(b['inputs']['features'][i, :lens[i]], feats[i])
    assert data.readers[1].sequence_length(data.elements[2][1]) == 12


def test_frame_targets_batch_contract_and_unchanged_defaults():
    from nabu_amd.processing.synthetic import SyntheticData
    d = SyntheticData(6, 50, 123, num_labels=3100, min_frames=20, frame_targets=True, target_name='alignments', seed=9)
    b = d.batch(2)
    n = b['input_seq_length']['features']
    y, m = b['targets']['alignments'], b['target_seq_length']['alignments']
    assert y.shape == (6, 50) and y.dtype == np.int32 and np.array_equal(m, n)
    assert y.max() < 3100 and y.min() >= 0 and len(np.unique(y)) > 50
    for i in range(6):
        assert np.all(y[i, n[i]:] == 0)
    assert np.array_equal(y, d.batch(2)['targets']['alignments'])
    assert d.validation(2).frame_targets
    # every existing argument combination draws what it drew before (same streams, same order)
    for kw in (dict(), dict(eos=True, min_labels=3, max_labels=6), dict(time_reduction=8, min_labels=2, max_labels=10)):
        new = SyntheticData(4, 80, 40, min_frames=40, seed=3, **kw).batch(1)
        old = SyntheticData(4, 80, 40, min_frames=40, seed=3, frame_targets=False, **kw).batch(1)
        for k in new:
            for name in new[k]:
                assert np.array_equal(new[k][name], old[k][name])
    # frame targets do not move the features or the lengths of a batch
    a = SyntheticData(4, 80, 40, min_frames=40, seed=3).batch(1)
    f = SyntheticData(4, 80, 40, min_frames=40, seed=3, frame_targets=True).batch(1)
    assert np.array_equal(a['inputs']['features'], f['inputs']['features'])
    assert np.array_equal(a['input_seq_length']['features'], f['input_seq_length']['features'])


def test_ark_writer_layout(tmp_path):
    from nabu_amd.neuralnetworks.decoders.alignment_decoder import arkwrite
    scp, ark = str(tmp_path / 'feats.scp'), str(tmp_path / 'loglikes.ark')
    rng = np.random.default_rng(0)
    mats = {'spk1_utt1': rng.standard_normal((3, 5)).astype(np.float32),
            'u2': rng.standard_normal((1, 5)).astype(np.float32)}
    for k, v in mats.items():
        arkwrite(scp, ark, k, v)
    raw = open(ark, 'rb').read()
    assert raw[:len('spk1_utt1') + 5] == b'spk1_utt1\0BFM '                 # no space before the NUL (reference)
    assert raw[14:24] == struct.pack('<bibi', 4, 3, 4, 5)
    assert len(raw) == sum(len(k) + 15 + 4 * v.size for k, v in mats.items())
    lines = open(scp).read().splitlines()
    assert lines[0] == 'spk1_utt1 %s:9' % ark
    got = read_ark(scp)
    assert set(got) == set(mats) and all(np.array_equal(got[k], mats[k]) for k in mats)


def test_alignment_decoder_validation_and_prior(tmp_path, capsys):
    import configparser
    from nabu_amd.neuralnetworks.decoders.alignment_decoder import AlignmentDecoder

    class FakeModel(object):
        output_names = ['alignments']
        output_dims = {'alignments': 8}
    conf = configparser.ConfigParser()
    conf.read_dict({'decoder': {'decoder': 'alignment_decoder'}})
    dec = AlignmentDecoder(conf, FakeModel())
    assert dec.conf['prior'] == 'None'
    lp = dec.log_prior()
    assert 'WARNING could not find prior in file None using uniform prior' in capsys.readouterr().out
    assert np.allclose(lp, np.log(1.0 / 8))
    np.save(str(tmp_path / 'p.npy'), np.arange(1, 9) / 36.0)
    conf.set('decoder', 'prior', str(tmp_path / 'p.npy'))
    assert np.allclose(AlignmentDecoder(conf, FakeModel()).log_prior(), np.log(np.arange(1, 9) / 36.0))
    with pytest.raises(Exception, match='AlignmentDecoder can not be used to validate'):
        dec.update_evaluation_loss([0.0], {}, {}, {})


def test_splice_order_on_a_hand_built_input():
    """blocks 0, +1, -1, +2, -2 over the padded batch tensor (tests/dnn_ref.py is the GPU tests' reference)"""
    from tests import dnn_ref
    x = torch.arange(1, 6, dtype=torch.float64).reshape(1, 5, 1)          # frames 1..5, F = 1
    s = dnn_ref.splice(x, 3)[0].numpy()
    assert s.tolist() == [[1, 2, 0, 3, 0], [2, 3, 1, 4, 0], [3, 4, 2, 5, 1], [4, 5, 3, 0, 2], [5, 0, 4, 0, 3]]
    from nabu_amd.neuralnetworks.models.ed_encoders import dnn
    assert dnn.splice_ld(123, 5) == 1120 and dnn.splice_ld(13, 3) == 96


def test_dnn_symbols_declared_bound_and_wrapped_at_abi_version_4():
    import re
    from nabu_amd import _hip, ops
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nabu_hip.h')).read()
    for sym in ('nabu_splice_stack_f32', 'nabu_unstack_rows_f32', 'nabu_stack_rows_f32', 'nabu_rows_relu_ln_fwd',
                'nabu_rows_relu_ln_bwd', 'nabu_rows_relu_ln_bwd_parts', 'nabu_xent_wide_loss_grad',
                'nabu_xent_wide_ws_bytes', 'nabu_log_softmax_prior_f32'):
        assert re.search(r'\b%s\s*\(' % sym, hdr) and sym in _hip.SIGNATURES
    for fn in ('splice_stack', 'unstack_rows', 'stack_rows', 'rows_relu_ln_fwd', 'rows_relu_ln_bwd',
               'xent_wide_loss_grad', 'log_softmax_prior'):
        assert callable(getattr(ops, fn))
    from nabu_amd import build
    build.build(verbose=False)
    lib = _hip.lib()
    assert lib.nabu_version() == 4
    assert lib.nabu_xent_wide_ws_bytes(32, 1000) == 32 * 1000 * 4
    assert lib.nabu_rows_relu_ln_bwd_parts(10) == 10 and lib.nabu_rows_relu_ln_bwd_parts(10 ** 6) == 1024
    # host-side argument checks: no launch
    assert lib.nabu_rows_relu_ln_fwd(4, 10, None, None, None, 1e-12, None, None, None, None) == -2
    assert lib.nabu_rows_relu_ln_fwd(4, 8192, None, None, None, 1e-12, None, None, None, None) == -2
    assert lib.nabu_splice_stack_f32(2, 5, 3, 2, None, None, None, 8, None) == -1       # ld < (2c-1) F
    assert lib.nabu_xent_wide_loss_grad(1, 4, 3, 2, None, None, None, None, 1.0, None, None, None, 0, None) == -1
