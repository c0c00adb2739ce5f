"""One rank of a data-parallel run with clip_gradient_norm (started by tests/test_hip_grad_norm.py with RANK /
WORLD_SIZE / LOCAL_RANK / MASTER_PORT in the environment): a shrunken cfg2 on two ranks, one batch per rank and update.
A first run with a norm bound nothing reaches finds the gradient norms; c = half the smallest.  Then three updates with
the flat exchange and three with allreduce_buckets = True at that c, and — on every rank, without a process group — the
same three updates on one replica that takes both ranks' batches with numbatches_to_aggregate = 2.  flat, adam_m,
adam_v, the stats words, the losses and the norms of each run are written to <outdir>/rank<r>.npz."""
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


def run(data, server, rank, c, A, buckets=False):
    world = server.world_size if server is not None else 1
    over = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.clip_gradient_norm': c,
            'trainer.numbatches_to_aggregate': A * world, 'trainer.allreduce_buckets': str(buckets)}
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=server, task_index=rank)
    assert tr.accumulate == A and tr.clip_norm == c
    losses, norms, initial = [], [], None
    for update in range(UPDATES):
        batches = [tr.to_device(data.batch((update * A + j) * world + rank)) for j in range(A)]
        if initial is None:
            tr._create_graph()
            tr._ensure_variables()
            tr._init_optimizer()
            initial = tr.flat.cpu().numpy().copy()
        loss = tr.step(batches[0]) if A == 1 else tr.step_accumulated(batches)
        tr.global_step += 1
        losses.append(float(loss.item()))
        norms.append(tr.grad_stats()[0])
        assert (tr.buckets is not None) == buckets and tr._micro == 0
    torch.cuda.synchronize()
    return dict(flat=tr.flat.cpu().numpy(), adam_m=tr.adam_m.cpu().numpy(), adam_v=tr.adam_v.cpu().numpy(),
                stats=tr.clip_stats.cpu().numpy(), losses=np.array(losses), norms=np.array(norms)), initial


def main():
    outdir = sys.argv[1]
    server = dist.create_server()
    rank = server.rank
    assert server.world_size == 2
    data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11)
    probe, initial = run(data, server, rank, 1e30, 1)
    c = 0.5 * float(probe['norms'].min())
    out = {'c': np.float64(c), 'initial': initial}
    for mode in ('flat', 'buckets'):
        res, _ = run(data, server, rank, c, 1, buckets=mode == 'buckets')
        out.update({mode + '/' + k: v for k, v in res.items()})
    server.barrier()
    # one replica, both ranks' batches per update (the ranks share the device, so the layers of this process run the
    # same kernels as before)
    res, _ = run(data, None, 0, c, 2)
    out.update({'single/' + k: v for k, v in res.items()})
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **out)
    server.barrier()
    server.shutdown()


if __name__ == '__main__':
    main()
