"""One rank of a data-parallel run with weight noise (started by tests/test_hip_weight_noise.py with RANK / WORLD_SIZE /
LOCAL_RANK / MASTER_PORT in the environment): a shrunken cfg2 with trainer.weight_noise = 0.075, two noisy clip+Adam
steps on this rank's own batches with the plain exchange and two with allreduce_buckets = True, then every variable of
both trainers written to <outdir>/rank<r>.npz."""
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

STEPS = 2


def main():
    outdir = sys.argv[1]
    server = dist.create_server()
    rank, world = server.rank, server.world_size
    data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11)
    out = {}
    for mode in ('plain', 'buckets'):
        over = {'encoder.num_units': 16, 'trainer.batch_size': 3, 'trainer.weight_noise': 0.075,
                'trainer.allreduce_buckets': str(mode == 'buckets')}
        mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
        tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                 server=server, task_index=rank)
        losses, noisy = [], []
        for step in range(STEPS):
            before = tr.last_weight_noise
            losses.append(float(tr.step(tr.to_device(data.batch(step * world + rank))).item()))
            tr.global_step += 1
            noisy.append(int(tr.last_weight_noise is not None and tr.last_weight_noise != before))
            if step == 0 and mode == 'buckets':
                assert tr.buckets is not None
        torch.cuda.synchronize()
        out['__losses_' + mode], out['__noisy_' + mode] = np.array(losses), np.array(noisy)
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
