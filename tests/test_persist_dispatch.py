"""The persistent recurrence's launch plan decides what it decided before it existed: the size and query exports of a
BLSTM layer over a grid of descriptors and under every NABU_PERSIST_* switch (tools/persist_dispatch_table.py) against
tables recorded from the library of the commit BEFORE the plan was introduced (each golden's "note" names it) — without
a device (exact-fp32 geometry, default CU count) and on a whole MI355X."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import persist_dispatch_table as pdt                 # noqa: E402


def _compare(name, extra):
    with open(os.path.join(ROOT, 'tests', 'golden', name)) as fid:
        want = pdt.expand(json.load(fid))
    got = pdt.table(extra)
    assert len(got['']) == 26400 and set(got) == set(pdt.ENVS)
    msgs = pdt.differences(got, want)
    assert not msgs, '\n'.join(msgs)


def test_dispatch_table_without_a_device():
    _compare('persist_dispatch_cpu.json', pdt.NO_DEVICE)


@pytest.mark.gpu
def test_dispatch_table_on_a_whole_mi355x():
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count < 256:
        pytest.skip('the golden was recorded on a whole MI355X (256 CUs)')
    _compare('persist_dispatch_mi355x.json', None)
