"""CPU: the packed batch layout (processing/prefetch.py) against a numpy restatement of nabu_batch_unpack, the
BatchPrefetcher's ordering / depth / reset / error / close contract over a recording fake source, RecordData read by
several threads, and the host-side argument errors of nabu_batch_unpack."""
import ctypes
import threading

import numpy as np
import pytest

from nabu_amd.processing import prefetch
from nabu_amd.processing.prefetch import BatchPrefetcher


def ragged_batch(rng, B, specs):
    """specs: (key, name, max_len, width); row 0 has the full length, row 1 (if any) length 0; zero padded"""
    out = dict(inputs={}, input_seq_length={}, targets={}, target_seq_length={})
    for key, name, T, F in specs:
        lens = rng.integers(0, T + 1, B).astype(np.int32)
        lens[0] = T
        if B > 1:
            lens[1] = 0
        if B > 2:
            lens[2] = 1
        shape = (B, T) if F == 1 else (B, T, F)
        if key == 'inputs':
            a = rng.standard_normal(shape).astype(np.float32)
        else:
            a = rng.integers(1, 1000, shape).astype(np.int32)
        mask = np.arange(T)[None, :] < lens[:, None]
        a = a * (mask if F == 1 else mask[:, :, None]).astype(a.dtype)
        out[key][name] = a
        out['input_seq_length' if key == 'inputs' else 'target_seq_length'][name] = lens
    return out


def test_packed_layout_round_trip():
    rng = np.random.default_rng(0)
    specs = [('inputs', 'a', 9, 40), ('inputs', 'b', 6, 123), ('targets', 'x', 5, 1), ('targets', 'y', 4, 3)]
    batch = ragged_batch(rng, 5, specs)
    assert batch['input_seq_length']['a'][1] == 0
    staged = prefetch.stage(batch)
    assert len(staged.segments) == 4 and staged.nbytes % 16 == 0 and staged.slot is None
    words = staged.array.view(np.int32)
    for s in staged.segments:
        assert s.data_off % 16 == 0 and s.len_off % 4 == 0 and s.row_off == s.len_off + 4 * s.rows
        lens = words[s.len_off // 4:s.len_off // 4 + s.rows]
        offs = words[s.row_off // 4:s.row_off // 4 + s.rows + 1]
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(lens.astype(np.int64) * s.width)]))
        assert s.data_off + 4 * offs[-1] <= staged.nbytes
    # no padding travels: the buffer is smaller than the padded tensors
    assert staged.nbytes < sum(a.nbytes for k in ('inputs', 'targets') for a in batch[k].values())
    got = prefetch.unpack_reference(staged)
    for key in ('inputs', 'targets', 'input_seq_length', 'target_seq_length'):
        assert set(got[key]) == set(batch[key])
        for name in batch[key]:
            assert got[key][name].dtype == batch[key][name].dtype and np.array_equal(got[key][name], batch[key][name])
    # the packer casts while it copies (float64 features, int64 labels), and packs into a slot that is large enough
    wide = {k: {n: (a.astype(np.float64) if k == 'inputs' else a.astype(np.int64)) if k in ('inputs', 'targets') else a
                for n, a in v.items()} for k, v in batch.items()}

    class Slot(object):
        array = np.zeros(staged.nbytes + 64, np.uint8)
    again = prefetch.stage(wide, Slot)
    assert again.array is Slot.array and again.nbytes == staged.nbytes
    got = prefetch.unpack_reference(again)
    for key in ('inputs', 'targets'):
        for name in batch[key]:
            assert got[key][name].dtype == batch[key][name].dtype and np.array_equal(got[key][name], batch[key][name])


class FakeSource(object):
    """records every request; batch k is {'step': k}; steps in `slow` wait for their gate, steps in `bad` raise"""

    def __init__(self, slow=(), bad=()):
        self.lock = threading.Lock()
        self.requested = []
        self.gates = {k: threading.Event() for k in slow}
        self.bad = set(bad)
        self.threads = set()
        self.returned = {}

    def batch(self, step):
        with self.lock:
            self.requested.append(step)
            self.threads.add(threading.current_thread().name)
            done = self.returned.setdefault(step, threading.Event())
        if step in self.gates:
            assert self.gates[step].wait(30)
        if step in self.bad:
            raise KeyError('step %d' % step)
        done.set()
        return {'step': step}

    def wait_returned(self, step):
        with self.lock:
            done = self.returned.setdefault(step, threading.Event())
        assert done.wait(30)


def live_workers():
    return [t for t in threading.enumerate() if t.name.startswith('nabu-prefetch')]


def test_prefetcher_order_depth_reset_errors_and_close():
    src = FakeSource(slow=(5,))
    pf = BatchPrefetcher(src, first_step=3, stride=2, depth=3, workers=3, stage=lambda b: dict(b, staged=True))
    try:
        # 5 is held back: 7 and 9 finish first, the consumer still receives 3, 5, 7 in order
        first = pf.get()
        assert first == {'step': 3, 'staged': True}
        assert max(src.requested) <= 3 + 2 * 3                   # at most `depth` ahead of the batch just handed out
        src.wait_returned(7), src.wait_returned(9)
        src.gates[5].set()
        assert [pf.get()['step'] for _ in range(3)] == [5, 7, 9]
        for k in (11, 13, 15):
            src.wait_returned(k)
        with src.lock:
            assert sorted(src.requested) ==list(range(3, 9 + 2 * 3 + 1, 2))
        assert threading.current_thread().name not in src.threads and len(live_workers()) == 3
        # reset: what was in flight is dropped, the stream continues at 40
        pf.reset(40)
        assert [pf.get()['step'] for _ in range(2)] == [40, 42] and pf.next_step == 44
        with src.lock:
            assert 17 not in src.requested
    finally:
        pf.close()
    assert live_workers() == []
    with pytest.raises(RuntimeError, match='closed'):
        pf.get()
    # a worker's exception surfaces at get() for its own step, after the earlier batches; the stream goes on behind it
    src = FakeSource(bad=(2,))
    pf = BatchPrefetcher(src, 0, 1, 2, 2, None)
    try:
        assert pf.get() == {'step': 0} and pf.get() == {'step': 1}
        with pytest.raises(KeyError, match='step 2'):
            pf.get()
        assert pf.get() == {'step': 3}
    finally:
        pf.close()
    assert live_workers() == []
    # worker counts: never more than 8, at least one
    pf = BatchPrefetcher(FakeSource(), 0, 1, 1, 64, None)
    n = len(live_workers())
    pf.close()
    assert n == prefetch.MAX_WORKERS == 8 and prefetch.DEFAULT_WORKERS == 2 and live_workers() == []


def test_prefetcher_with_a_slot_ring_recycles_slots_after_their_upload():
    """the ring logic without a device: slots whose 'event' has completed come back, a consumed batch whose upload was
    never recorded is an error instead of a dead wait"""
    class Event(object):
        def __init__(self):
            self.done = False

        def query(self):
            return self.done

        def synchronize(self):
            self.done = True

    ring = prefetch.PinnedRing(3)
    for s in ring.free:
        s.array = np.zeros(1 << 12, np.uint8)                    # stands for pinned memory
    src = FakeSource()

    def stage(batch, slot):
        b = dict(inputs={'f': np.full((1, 2, 4), batch['step'], np.float32)}, input_seq_length={'f': np.array([2], np.int32)},
                 targets={}, target_seq_length={})
        return prefetch.stage(b, slot)
    pf = BatchPrefetcher(src, 0, 1, 2, 2, stage, ring)
    try:
        for k in range(8):
            staged = pf.get()
            assert staged.slot is not None and staged.array is staged.slot.array
            assert prefetch.unpack_reference(staged)['inputs']['f'][0, 0, 0] == k
            staged.slot.uploaded(Event())                        # completes when somebody waits for it
        pf.reset(20)
        staged = pf.get()
        assert prefetch.unpack_reference(staged)['inputs']['f'][0, 0, 0] == 20
        with pytest.raises(RuntimeError, match='uploaded'):      # three slots, none handed back
            for _ in range(4):
                pf.get()
    finally:
        pf.close()
    assert live_workers() == []


def test_record_data_from_three_threads_equals_the_serial_batches(tmp_path):
    from tests.test_data_path import make_dataset
    from nabu_amd.processing import input_pipeline

    conf, _, _, _ = make_dataset(str(tmp_path / 'd'), n=23, dim=5)

    def source():
        return input_pipeline.from_sections(conf, ['features'], [['trainfbank']], ['text'], [['traintext']],
                                            batch_size=4, numbuckets=2, shuffle=True, seed=0)
    serial = source()
    steps = 2 * serial.num_batches() + 1                          # two epochs and the carry into the third
    want = [serial.batch(k) for k in range(steps)]
    serial.close()
    threaded = source()
    pf = BatchPrefetcher(threaded, 0, 1, 3, 3, None)
    try:
        assert threaded.lookahead is False
        got = [pf.get() for _ in range(steps)]
    finally:
        pf.close()
    assert threaded.lookahead is True and not threaded._ahead
    threaded.close()
    for w, g in zip(want, got):
        for key in w:
            assert set(w[key]) == set(g[key])
            for name in w[key]:
                assert np.array_equal(w[key][name], g[key][name])


def test_batch_unpack_argument_errors_on_the_host():
    """no GPU needed: nabu_batch_unpack validates before any launch"""
    from nabu_amd import _hip
    lib = _hip.lib()
    assert 'nabu_batch_unpack' in _hip.SIGNATURES and _hip.BATCH_MAX_SEGS == 8
    assert ctypes.sizeof(_hip.BatchSeg) == 56
    one = 4096                                                     # a non-null, aligned pointer: never touched

    def segs(n=1, **over):
        arr = (_hip.BatchSeg * max(n, 1))()
        for d in arr:
            d.rows, d.width, d.max_len = 2, 4, 3
            d.len_off, d.row_off, d.data_off = 0, 8, 32
            d.out, d.out_len = one, one
            for k, v in over.items():
                setattr(d, k, v)
        return ctypes.cast(arr, ctypes.c_void_p), arr

    def call(n, seg_ptr, packed, nbytes):
        return lib.nabu_batch_unpack(n, seg_ptr, packed, nbytes, None)
    p, keep = segs()
    assert call(1, None, one, 256) == -1 and b'null' in lib.nabu_last_error()
    assert call(1, p, None, 256) == -1 and b'null' in lib.nabu_last_error()
    p9, keep9 = segs(9)
    assert call(9, p9, one, 256) == -1 and b'nseg' in lib.nabu_last_error()
    assert call(0, p, one, 256) == -1 and b'nseg' in lib.nabu_last_error()
    for field in ('len_off', 'row_off', 'data_off'):
        p, keep = segs(**{field: 1 << 20})
        assert call(1, p, one, 256) == -1 and b'outside' in lib.nabu_last_error(), field
    p, keep = segs(row_off=248)                                   # 3 offsets of 4 bytes do not fit behind byte 248
    assert call(1, p, one, 256) == -1 and b'outside' in lib.nabu_last_error()
    for field, value in (('len_off', 2), ('row_off', 6), ('data_off', 40)):
        p, keep = segs(**{field: value})
        assert call(1, p, one, 256) == -1 and b'misaligned' in lib.nabu_last_error(), field
    p, keep = segs()
    assert call(1, p, one + 4, 256) == -1 and b'aligned' in lib.nabu_last_error()
    for field in ('rows', 'width', 'max_len'):
        for value in (0, -3):
            p, keep = segs(**{field: value})
            assert call(1, p, one, 256) == -1 and b'positive' in lib.nabu_last_error(), field
    for field in ('out', 'out_len'):
        p, keep = segs(**{field: None})
        assert call(1, p, one, 256) == -1 and b'null' in lib.nabu_last_error(), field
    p, keep = segs(rows=1 << 15, width=1 << 8, max_len=1 << 8)
    assert call(1, p, one, 1 << 30) == -1 and b'2^31' in lib.nabu_last_error()
    assert lib.nabu_version() == 4
