"""One rank of a data-parallel run with gradient accumulation (started by tests/test_hip_grad_accum.py with RANK /
WORLD_SIZE / LOCAL_RANK / MASTER_PORT in the environment): a shrunken cfg2 with numbatches_to_aggregate = 4 on two
ranks, so two micro-batches per rank and update; two updates on this rank's own batches with the flat exchange and two
with allreduce_buckets = True, then every variable of both trainers, the losses and the number of gradient exchanges
per update written to <outdir>/rank<r>.npz."""
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

UPDATES = 2


def main():
    outdir = sys.argv[1]
    server = dist.create_server()
    rank, world = server.rank, server.world_size
    data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11)
    exchanges = [0]
    for name in ('all_reduce_sum_', 'all_reduce_sum_async'):
        def counted(t, _fn=getattr(server, name)):
            if t.numel() > 1:                      # (a gradient, not a loss)
                exchanges[0] += 1
            return _fn(t)
        setattr(server, name, counted)
    out = {}
    for mode in ('flat', 'buckets'):
        over = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.numbatches_to_aggregate': 2 * world,
                'trainer.allreduce_buckets': str(mode == 'buckets')}
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                 server=server, task_index=rank)
        A = tr.accumulate
        assert A == 2
        losses, counts = [], []
        for update in range(UPDATES):
            exchanges[0] = 0
            batches = [tr.to_device(data.batch((update * A + j) * world + rank)) for j in range(A)]
            losses.append(float(tr.step_accumulated(batches).item()))
            tr.global_step += 1
            counts.append(exchanges[0])
            assert (tr.buckets is not None) == (mode == 'buckets') and tr._micro == 0
        torch.cuda.synchronize()
        out['__losses_' + mode], out['__exchanges_' + mode] = np.array(losses), np.array(counts)
        for name, value in tr.model.store.state_dict().items():
            out[mode + '/' + name] = value
        if mode == 'buckets':
            fresh = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                        server=None, task_index=0)
            fresh._create_graph()
            fresh._ensure_variables()
            torch.cuda.synchronize()
            for name, value in fresh.model.store.state_dict().items():
                out['__initial/' + name] = value
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), **out)
    server.barrier()
    server.shutdown()


if __name__ == '__main__':
    main()
