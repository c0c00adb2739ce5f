"""GPU: nabu_batch_unpack (csrc/batch.hip) against Trainer.to_device on the same numpy batch — bit for bit, length
tensors included — over a grid of shapes that takes both access widths (16 bytes for width % 4 == 0, 4 bytes else),
rows of length 0, 1 and max_len, and more than one workgroup; one full-size batch; and a corrupt length, which is
clamped and writes nothing outside its output."""
import numpy as np
import pytest
import torch

from nabu_amd import ops, recipes
from nabu_amd.processing import prefetch
from nabu_amd.processing.synthetic import SyntheticData
from tests.test_prefetch import ragged_batch

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope='module')
def trainer():
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **{'encoder.num_units': 16})
    return trainer_factory.factory('standard')(conf=tc, dataconf=SyntheticData(2, 16, 40), modelconf=mc,
                                               evaluatorconf=ec, expdir=None, server=None, task_index=0)


def unpack_into_guarded(staged, shift=0):
    """ops.batch_unpack into pre-filled outputs (NaN / -1) with GUARD untouched-or-else elements behind each;
    `shift` moves every output off its 16-byte alignment"""
    dev = torch.device('cuda')
    packed = torch.from_numpy(staged.array[:staged.nbytes].copy()).to(dev)
    segs, outs = [], []
    for s in staged.segments:
        n = s.rows * s.max_len * s.width
        fill = float('nan') if s.key == 'inputs' else -1
        dtype = torch.float32 if s.key == 'inputs' else torch.int32
        data = torch.full((shift + n + GUARD,), fill, dtype=dtype, device=dev)
        lens = torch.full((s.rows + GUARD,), -1, dtype=torch.int32, device=dev)
        segs.append(s.describe() + (data[shift:shift + n], lens[:s.rows]))
        outs.append((s, data, lens, n))
    ops.batch_unpack(segs, packed, staged.nbytes)
    torch.cuda.synchronize()
    got = dict(inputs={}, targets={}, input_seq_length={}, target_seq_length={})
    for s, data, lens, n in outs:
        guard, lguard = data[shift + n:].cpu().numpy(), lens[s.rows:].cpu().numpy()
        head = data[:shift].cpu().numpy()
        if s.key == 'inputs':
            assert np.isnan(guard).all() and np.isnan(head).all(), s.name
        else:
            assert (guard == -1).all() and (head == -1).all(), s.name
        assert (lguard == -1).all(), s.name
        got[s.key][s.name] = data[shift:shift + n].view(s.shape)
        got['input_seq_length' if s.key == 'inputs' else 'target_seq_length'][s.name] = lens[:s.rows]
    return got


def assert_same(got, want):
    """want: Trainer.to_device's result"""
    for key in ('inputs', 'targets'):
        assert set(got[key]) == set(want[key])
        for name, w in want[key].items():
            g = got[key][name]
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (key, name)
    for key in ('input_seq_length', 'target_seq_length'):
        for name, w in want[key].items():
            g = got[key][name]
            g = g.dev if hasattr(g, 'dev') else g
            assert g.dtype == torch.int32 and torch.equal(g, w.dev), (key, name)
            if hasattr(got[key][name], 'host'):
                assert np.array_equal(got[key][name].host, w.host)


@pytest.mark.parametrize('T', [1, 7, 65])
@pytest.mark.parametrize('B', [1, 5, 33])
def test_unpack_equals_to_device(trainer, B, T):
    rng = np.random.default_rng(1000 * B + T)
    T2 = {1: 7, 7: 65, 65: 1}[T]
    for wa, wb, wx, wy in ((40, 123, 1, 3), (1, 3, 40, 123)):          # every width as features and as labels
        batch = ragged_batch(rng, B, [('inputs', 'a', T, wa), ('inputs', 'b', T2, wb),
                                      ('targets', 'x', T2, wx), ('targets', 'y', T, wy)])
        want = trainer.to_device(batch)
        staged = trainer.stage(batch)
        assert len(staged.segments) == 4
        assert_same(unpack_into_guarded(staged), want)
        assert_same(unpack_into_guarded(staged, shift=1), want)           # unaligned outputs: the 4-byte path
        assert_same(trainer.to_device_staged(staged), want)


def test_full_size_batch(trainer):
    batch = SyntheticData(32, 1000, 40, min_frames=300).batch(5)
    want = trainer.to_device(batch)
    staged = trainer.stage(batch)
    assert staged.nbytes < batch['inputs']['features'].nbytes               # the padding does not travel
    assert_same(unpack_into_guarded(staged), want)
    assert_same(trainer.to_device_staged(staged), want)


def test_corrupt_lengths_are_clamped(trainer):
    rng = np.random.default_rng(3)
    batch = ragged_batch(rng, 5, [('inputs', 'a', 7, 40), ('inputs', 'b', 7, 3), ('targets', 'x', 6, 1)])
    want = trainer.to_device(batch)
    staged = trainer.stage(batch)
    words = staged.array.view(np.int32)
    for s in staged.segments:
        words[s.len_off // 4 + 3] = s.max_len + 100000                      # far beyond the row and the buffer
        words[s.len_off // 4 + 4] = -7
    got = unpack_into_guarded(staged)                                       # asserts the guards
    for s in staged.segments:
        lkey = 'input_seq_length' if s.key == 'inputs' else 'target_seq_length'
        lens = got[lkey][s.name].cpu().numpy()
        assert lens[3] == s.max_len and lens[4] == 0
        assert np.array_equal(lens[:3], want[lkey][s.name].host[:3])
        g, w = got[s.key][s.name], want[s.key][s.name]
        assert torch.equal(g[:3], w[:3])                                    # the rows with honest lengths
        assert not bool((g[4] != 0).any())                                  # a negative length is a row of zeros
        # row 3 holds whatever lies behind its offset inside the packed buffer, or zeros where that would leave it:
        # every element of it was written (as a float, a -7 length word of a later segment's header reads as a NaN)
        left = (torch.isnan(g[3]) if s.key == 'inputs' else g[3] == -1).sum()
        assert int(left) <= (len(staged.segments) if s.key == 'inputs' else 0)
