"""One rank of a data-parallel run with the auxiliary CTC loss (started by tests/test_hip_joint_ctc.py with RANK /
WORLD_SIZE / LOCAL_RANK / MASTER_PORT in the environment): a shrunken cfg3 with ctc_head = True and ctc_weight = 0.3 on
two ranks, one batch per rank and update.  Three updates with the flat exchange and three with allreduce_buckets =
True.  flat, adam_m, adam_v, the losses and the bucket each variable went to are written to <outdir>/rank<r>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nabu_amd import recipes                                                  # noqa: E402
from nabu_amd.computing import dist                                           # noqa: E402
from nabu_amd.neuralnetworks.trainers import trainer_factory                  # noqa: E402
from nabu_amd.processing.synthetic import SyntheticData                       # noqa: E402

UPDATES = 3


def run(data, server, rank, buckets):
    over = {'encoder.num_units': 16, 'decoder.num_units': 16, 'trainer.batch_size': 3, 'decoder.ctc_head': 'True',
            'trainer.ctc_weight': 0.3, 'trainer.allreduce_buckets': str(buckets)}
    mc, tc, ec = recipes.load_recipe('cfg3_las_vanilla', **over)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=server, task_index=rank)
    assert tr.ctc_weight == 0.3
    losses, initial = [], None
    for update in range(UPDATES):
        batch = tr.to_device(data.batch(update * server.world_size + rank))
        if initial is None:
            tr._create_graph()
            tr._ensure_variables()
            tr._init_optimizer()
            initial = tr.flat.cpu().numpy().copy()
        losses.append(float(tr.step(batch).item()))
        tr.global_step += 1
        assert (tr.buckets is not None) == buckets
    torch.cuda.synchronize()
    head = [v for v in tr.model.store.trainable_variables() if '/ctc_outlayer/' in v.name]
    assert len(head) == 2
    out = dict(flat=tr.flat.cpu().numpy(), adam_m=tr.adam_m.cpu().numpy(), adam_v=tr.adam_v.cpu().numpy(),
               losses=np.array(losses), initial=initial,
               head=np.concatenate([v.data.cpu().numpy().ravel() for v in head]),
               head_initial=np.concatenate([initial[v.offset:v.offset + v.numel()] for v in head]))
    if buckets:       # the key of the bucket that holds the head's variables
        keys = [b['key'] for b in tr.buckets if any(v is h for v in b['vars'] for h in head)]
        out['head_buckets'] = np.array(keys)
    return out


def main():
    outdir = sys.argv[1]
    server = dist.create_server()
    rank = server.rank
    assert server.world_size == 2
    data = SyntheticData(3, 32, 40, min_frames=24, min_labels=1, max_labels=2, eos=True, time_reduction=8, seed=11)
    out = {}
    for mode in ('flat', 'buckets'):
        res = run(data, server, rank, mode == 'buckets')
        out.update({mode + '/' + k: v for k, v in res.items()})
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **out)
    server.barrier()
    server.shutdown()


if __name__ == '__main__':
    main()
