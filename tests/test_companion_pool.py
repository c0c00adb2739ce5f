"""The buffers behind the packed companions (nabu_amd/neuralnetworks/components/ops.py, BufferPool): a slot is busy
exactly while the view it handed out is alive, a free slot of the same size and layout is reused, and a new size frees
the idle ones, so what a key holds is bounded by its live holders and not by the shapes it has seen.  The per-tensor
metadata (value bound, packed companion) lives and dies with the tensor object.  CPU tensors, no HIP library."""
import gc

import numpy as np
import torch

from nabu_amd.neuralnetworks.components import ops

CPU = torch.device('cpu')


def test_a_free_slot_of_the_same_size_is_reused():
    pool = ops.BufferPool()
    a = pool.acquire(('L', 'hT'), 256, CPU, (4, 8))
    ptr = a.data_ptr()
    a.fill_(7)                          # (a user's content: the slot is rewritten in full by its next user)
    del a
    b = pool.acquire(('L', 'hT'), 256, CPU, (4, 8))
    assert b.data_ptr() == ptr and b.numel() == 256 and b.dtype == torch.uint8
    assert pool.held_bytes('hT') == 256


def test_a_held_slot_is_not_handed_out_again():
    pool = ops.BufferPool()
    a = pool.acquire(('L', 'hT'), 256, CPU)
    b = pool.acquire(('L', 'hT'), 256, CPU)
    assert a.data_ptr() != b.data_ptr() and not a.any() and not b.any()
    assert pool.held_bytes('hT') == 512
    keep = [a]                          # any holder keeps the slot busy (a plan's _keep, a packed() companion)
    del a, b
    c = pool.acquire(('L', 'hT'), 256, CPU)
    assert c.data_ptr() != keep[0].data_ptr()
    assert pool.held_bytes('hT') == 512


def test_a_new_size_or_layout_frees_the_idle_slots_of_its_key_only():
    pool = ops.BufferPool()
    held = pool.acquire(('L', 'rows'), 100, CPU, (1,))
    idle = pool.acquire(('L', 'rows'), 100, CPU, (1,))
    other = pool.acquire(('M', 'rows'), 100, CPU, (1,))
    del idle, other
    assert pool.held_bytes('rows') == 300
    new = pool.acquire(('L', 'rows'), 300, CPU, (3,))
    assert pool.held_bytes('rows') == 100 + 300 + 100      # the held slot and the other key's idle one stay
    del new
    same_size = pool.acquire(('L', 'rows'), 300, CPU, (4,))  # equal size, another layout: not reused
    assert pool.held_bytes('rows') == 100 + 300 + 100 and held.numel() == 100
    assert not same_size.any()


def test_random_sizes_without_holders_keep_one_buffer_per_key():
    pool = ops.BufferPool()
    rng = np.random.default_rng(0)
    last = {}
    for _ in range(50):
        for role in ('rows', 'cols', 'hT'):
            n = int(rng.integers(1, 8)) * 16
            buf = pool.acquire(('L', role), n, CPU, (n,))
            assert buf.numel() == n and (n == last.get(role) or not buf.any())     # (a new buffer is zero-filled)
            last[role] = n
            buf.fill_(1)
            del buf
            assert pool.held_bytes(role) == n                   # the last buffer alone
    assert pool.held_bytes() == sum(last.values())


def test_metadata_lives_and_dies_with_the_tensor_and_views_do_not_inherit_it():
    t = torch.zeros(4, 6)
    assert ops.value_bound(t) == 0.0 and ops.packed(t, 1) is None
    rows, cols = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)
    ops.set_value_bound(t, 1.0)
    ops.set_packed(t, 2, (rows, cols))
    assert ops.value_bound(t) == 1.0
    assert ops.packed(t, 2) == (rows, cols) and ops.packed(t, 1) is None
    v = t.view(2, 12)
    assert ops.value_bound(v) == 0.0 and ops.packed(v, 2) is None
    pool = ops.BufferPool()
    lease = pool.acquire(('L', 'rows'), 8, CPU)
    ops.set_packed(t, 1, (lease, lease))
    ptr = lease.data_ptr()
    del lease, v
    assert pool.acquire(('L', 'rows'), 8, CPU).data_ptr() != ptr    # the tensor holds its companion's slot ...
    del t
    gc.collect()
    for _ in range(4):                                              # ... and a tensor made after it knows of none
        u = torch.zeros(4, 6)
        assert ops.value_bound(u) == 0.0 and ops.packed(u, 1) is None and ops.packed(u, 2) is None
    assert pool.acquire(('L', 'rows'), 8, CPU).data_ptr() == ptr    # ... until it is gone
