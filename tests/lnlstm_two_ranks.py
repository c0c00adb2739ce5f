"""One rank of a data-parallel run with layer-normalised layers (started by tests/test_hip_lnlstm.py with RANK /
WORLD_SIZE / LOCAL_RANK / MASTER_PORT in the environment): a shrunken cfg2 with encoder.layer_norm = True, a few
clip+Adam steps on this rank's own batches, then every variable written to <outdir>/rank<r>.npz."""
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

STEPS = 3


def main():
    outdir = sys.argv[1]
    server = dist.create_server()
    rank, world = server.rank, server.world_size
    over = {'encoder.num_units': 16, 'encoder.layer_norm': 'True', 'trainer.batch_size': 3}
    data = SyntheticData(3, 32, 40, min_frames=20, min_labels=2, max_labels=3, time_reduction=8, seed=11)
    mc, tc, ec = recipes.load_recipe('cfg2_listener_ctc', **over)
    tr = trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                             server=server, task_index=rank)
    losses = []
    for step in range(STEPS):
        losses.append(float(tr.step(tr.to_device(data.batch(step * world + rank))).item()))
    torch.cuda.synchronize()
    state = tr.model.store.state_dict()
    np.savez(os.path.join(outdir, 'rank%d.npz' % rank), __losses=np.array(losses), **state)
    server.barrier()
    server.shutdown()


if __name__ == '__main__':
    main()
