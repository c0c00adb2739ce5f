"""Batches assembled ahead of the training step, and the packed form a batch travels in.

Two parts:

* the PACKED LAYOUT of a batch (`layout`, `pack`, `unpack_reference`): what nabu_batch_unpack (csrc/batch.hip,
  include/nabu_hip.h) reads.  Every tensor of the batch contract (each input, each target) is one segment:
  B int32 lengths, B + 1 int32 element offsets of its rows (the prefix sum of len[b] * width, so the device needs no
  scan), and the rows back to back without their padding as 4-byte elements (float32 features, int32 labels: the
  packer casts while it copies), the row data starting 16-byte aligned.  One upload and one launch then replace one
  blocking copy per tensor and per length vector.  The padding of a batch is zero by contract (synthetic.py,
  input_pipeline.py); the unpacked batch has zeros there whatever the source held.

* `BatchPrefetcher`: worker threads call a batch source for steps first_step, first_step + stride, ... and stage each
  batch (pack it into a pinned slot) while the device trains; the consumer receives them strictly in order.  Workers
  never call into HIP or torch's device API: pinned slots are allocated, grown and recycled on the consumer's thread
  (`PinnedRing`), a slot returns to the ring only after the event recorded behind its upload has completed."""
import collections
import threading

import numpy as np

MAX_WORKERS = 8            # a GPU host grants this process a few CPUs out of many: never sized from os.cpu_count()
DEFAULT_WORKERS = 2


def _align(n, a):
    return (n + a - 1) // a * a


class Segment(object):
    """one tensor of the packed batch: where it lies in the buffer and what it unpacks to"""
    __slots__ = ('key', 'name', 'shape', 'dtype', 'rows', 'width', 'max_len', 'len_off', 'row_off', 'data_off', 'lengths')

    def describe(self):
        return (self.rows, self.width, self.max_len, self.len_off, self.row_off, self.data_off)


class StagedBatch(object):
    """a packed batch: `array` (uint8 numpy view of the bytes, pinned when it lies in a ring slot), `nbytes`, the
    segments, and the slot it occupies (None outside a ring)"""

    def __init__(self, array, nbytes, segments, slot=None):
        self.array, self.nbytes, self.segments, self.slot = array, nbytes, segments, slot


_KEYS = (('inputs', 'input_seq_length', np.float32), ('targets', 'target_seq_length', np.int32))


def layout(batch):
    """(segments, nbytes) of a numpy batch (A0 contract: inputs / input_seq_length / targets / target_seq_length)"""
    segments, pos = [], 0
    for key, lkey, dtype in _KEYS:
        for name, a in batch[key].items():
            a = np.asarray(a)
            if a.ndim < 2 or a.size == 0:
                raise ValueError('%s[%s]: a batch tensor is [batch, time, ...] and not empty, got shape %s'
                                 % (key, name, a.shape))
            s = Segment()
            s.key, s.name, s.shape, s.dtype = key, name, tuple(a.shape), dtype
            s.rows, s.max_len = a.shape[0], a.shape[1]
            s.width = int(np.prod(a.shape[2:], dtype=np.int64))
            s.lengths = np.ascontiguousarray(np.asarray(batch[lkey][name], dtype=np.int32))
            if s.lengths.shape != (s.rows,):
                raise ValueError('%s[%s]: %d lengths for %d rows' % (lkey, name, s.lengths.size, s.rows))
            s.len_off = pos
            s.row_off = pos + 4 * s.rows
            s.data_off = _align(s.row_off + 4 * (s.rows + 1), 16)
            kept = np.clip(s.lengths, 0, s.max_len).astype(np.int64)
            pos = _align(s.data_off + 4 * int(kept.sum()) * s.width, 16)
            segments.append(s)
    return segments, pos


def pack(batch, segments, out):
    """write the packed form of `batch` into the uint8 array `out` (at least the layout's nbytes long)"""
    words = out[:len(out) // 4 * 4].view(np.int32)
    for s in segments:
        a = np.asarray(batch[s.key][s.name]).reshape(s.rows, s.max_len * s.width)
        kept = np.clip(s.lengths, 0, s.max_len).astype(np.int64) * s.width
        offs = np.zeros(s.rows + 1, np.int64)
        np.cumsum(kept, out=offs[1:])
        words[s.len_off // 4:s.len_off // 4 + s.rows] = s.lengths
        words[s.row_off // 4:s.row_off // 4 + s.rows + 1] = offs
        data = words[s.data_off // 4:s.data_off // 4 + int(offs[-1])].view(s.dtype)
        for b in range(s.rows):
            data[offs[b]:offs[b + 1]] = a[b, :kept[b]]           # casts to float32 / int32 while it copies


def stage(batch, slot=None):
    """numpy batch -> StagedBatch, packed into `slot` (a PinnedRing slot) when it is large enough, else into host
    memory of its own (the consumer's thread then grows the slot: BatchPrefetcher.get)"""
    segments, nbytes = layout(batch)
    if slot is not None and slot.array is not None and len(slot.array) >= nbytes:
        array = slot.array
    else:
        array = np.empty(nbytes, np.uint8)
    pack(batch, segments, array)
    return StagedBatch(array, nbytes, segments, slot)


def unpack_reference(staged):
    """numpy restatement of nabu_batch_unpack: the padded batch a StagedBatch unpacks to"""
    words = np.asarray(staged.array[:staged.nbytes]).view(np.int32)
    out = dict(inputs={}, input_seq_length={}, targets={}, target_seq_length={})
    for s in staged.segments:
        lens = words[s.len_off // 4:s.len_off // 4 + s.rows]
        offs = words[s.row_off // 4:s.row_off // 4 + s.rows + 1]
        data = words[s.data_off // 4:].view(s.dtype)
        pad = np.zeros((s.rows, s.max_len * s.width), s.dtype)
        kept = np.clip(lens, 0, s.max_len)
        for b in range(s.rows):
            n = int(kept[b]) * s.width
            pad[b, :n] = data[offs[b]:offs[b] + n]
        out[s.key][s.name] = pad.reshape(s.shape)
        out['input_seq_length' if s.key == 'inputs' else 'target_seq_length'][s.name] = kept.astype(np.int32)
    return out


class _Slot(object):
    def __init__(self):
        self.tensor = None         # pinned uint8 torch tensor (grow-only)
        self.array = None          # its numpy view: what a worker writes into
        self.event = None          # recorded behind the upload that reads the slot

    def ensure(self, nbytes):
        """consumer's thread only: pinned memory is allocated through the device runtime"""
        import torch
        if self.tensor is None or self.tensor.numel() < nbytes:
            self.tensor = torch.empty(_align(nbytes + nbytes // 4, 4096), dtype=torch.uint8, pin_memory=True)
            self.array = self.tensor.numpy()

    def uploaded(self, event):
        self.event = event


class PinnedRing(object):
    """`n` pinned staging slots; all methods belong to the consumer's thread"""

    def __init__(self, n):
        self.free = [_Slot() for _ in range(n)]
        self.busy = collections.deque()          # handed to the consumer: free again when their event has completed

    def take(self):
        while self.busy and self.busy[0].event is not None and self.busy[0].event.query():
            self._release(self.busy.popleft())
        return self.free.pop() if self.free else None

    def wait_oldest(self):
        """block until the oldest upload has completed and take its slot back"""
        if not self.busy or self.busy[0].event is None:
            raise RuntimeError('no staging slot is free and none is behind an upload: a staged batch was consumed '
                               'without slot.uploaded(event)')
        slot = self.busy.popleft()
        slot.event.synchronize()
        self._release(slot)

    def _release(self, slot):
        slot.event = None
        self.free.append(slot)


class _Task(object):
    __slots__ = ('step', 'generation', 'slot', 'done', 'result', 'error')


class BatchPrefetcher(object):
    """source.batch(step) for step = first_step, first_step + stride, ... computed by `workers` threads, at most `depth`
    batches ahead of the one the consumer holds, each passed through `stage` on the worker's thread.

    get()            the next staged batch, in order; an exception a worker hit is raised here, for its own step
    reset(step)      drop everything in flight and continue at `step` (go-back, restore)
    close()          join the threads
    A source with a thread-safe `assemble(step)` (input_pipeline.RecordData) is read through it, with its own one-batch
    look-ahead switched off for the prefetcher's lifetime.  With a `ring` every task owns one of its slots and `stage` is
    called as stage(batch, slot)."""

    def __init__(self, source, first_step, stride=1, depth=2, workers=DEFAULT_WORKERS, stage=None, ring=None):
        self.source = source
        self._fetch = getattr(source, 'assemble', None) or source.batch
        self._lookahead = getattr(source, 'lookahead', None) if hasattr(source, 'assemble') else None
        if self._lookahead is not None:
            source.lookahead = False
        self.stride, self.depth = max(int(stride), 1), max(int(depth), 1)
        self._stage, self.ring = stage, ring
        self._cond = threading.Condition()
        self._todo = collections.deque()
        self._tasks = collections.OrderedDict()     # step -> task, in submission order
        self._generation = 0
        self._started = set()                       # tasks a worker is computing
        self._stale_slots = []                      # slots of abandoned tasks a worker has finished with
        self._running_stale = 0
        self._closed = False
        self.next_step = int(first_step)            # the step get() returns next
        self._submit_step = self.next_step
        self._threads = [threading.Thread(target=self._work, name='nabu-prefetch-%d' % i, daemon=True)
                         for i in range(min(max(int(workers), 1), MAX_WORKERS))]
        for t in self._threads:
            t.start()
        with self._cond:
            self._fill()

    # -- consumer's thread
    def _fill(self):
        """submit until `depth` batches are in flight (or the ring has no free slot); called with the lock held"""
        if self.ring is not None and self._stale_slots:
            self.ring.free.extend(self._stale_slots)
            self._stale_slots = []
        while len(self._tasks) < self.depth and not self._closed:
            slot = None
            if self.ring is not None:
                slot = self.ring.take()
                if slot is None:
                    return
            t = _Task()
            t.step, t.generation, t.slot, t.done, t.result, t.error = self._submit_step, self._generation, slot, False, None, None
            self._tasks[t.step] = t
            self._todo.append(t)
            self._submit_step += self.stride
            self._cond.notify_all()

    def get(self):
        with self._cond:
            if self._closed:
                raise RuntimeError('the prefetcher is closed')
            while True:
                self._fill()
                head = self._tasks.get(self.next_step)
                if head is not None and head.done:
                    break
                if head is None and self.ring is not None and not self._running_stale:
                    # every slot is behind an upload: wait for the oldest one (without the lock: workers go on)
                    self._cond.release()
                    try:
                        self.ring.wait_oldest()
                    finally:
                        self._cond.acquire()
                    continue
                self._cond.wait()
            del self._tasks[self.next_step]
            self.next_step += self.stride
            if head.error is not None:
                if head.slot is not None:
                    self.ring.free.append(head.slot)
                self._fill()
                raise head.error
            staged = head.result
            if head.slot is not None and isinstance(staged, StagedBatch):
                if staged.array is not head.slot.array:       # the slot was too small: grow it here, not in the worker
                    head.slot.ensure(staged.nbytes)
                    head.slot.array[:staged.nbytes] = staged.array[:staged.nbytes]
                    staged.array = head.slot.array
                self.ring.busy.append(head.slot)
            elif head.slot is not None:
                self.ring.free.append(head.slot)
            self._fill()
            return staged

    def reset(self, next_step):
        with self._cond:
            self._generation += 1
            self._todo.clear()
            for t in self._tasks.values():
                if t.done or t not in self._started:
                    if t.slot is not None:
                        self.ring.free.append(t.slot)
                else:
                    self._running_stale += 1     # its worker hands the slot back when it is through
            self._tasks.clear()
            self._started.clear()
            self.next_step = self._submit_step = int(next_step)
            self._fill()

    def close(self):
        with self._cond:
            if self._closed:
                return
            self._closed = True
            self._generation += 1
            self._todo.clear()
            self._tasks.clear()
            self._cond.notify_all()
        for t in self._threads:
            t.join()
        if self._lookahead is not None:
            self.source.lookahead = self._lookahead

    # -- worker threads
    def _work(self):
        while True:
            with self._cond:
                while not self._todo and not self._closed:
                    self._cond.wait()
                if self._closed:
                    return
                task = self._todo.popleft()
                self._started.add(task)
            result = error = None
            try:
                result = self._fetch(task.step)
                if self._stage is not None:
                    result = self._stage(result) if self.ring is None else self._stage(result, task.slot)
            except Exception as e:               # raised again at get(), for this step
                error = e
            with self._cond:
                if task.generation != self._generation:
                    if not self._closed:
                        self._running_stale -= 1
                        if task.slot is not None:
                            self._stale_slots.append(task.slot)
                else:
                    task.result, task.error, task.done = result, error, True
                    self._started.discard(task)
                self._cond.notify_all()
