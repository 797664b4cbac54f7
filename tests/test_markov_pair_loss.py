"""Grid2DMarkovExperiment.pair_loss: the loss of one x / y pair batch without an optimisation step, which the CLI's `valid_loss`
of a pair batch is.  The value equals, to the bit, what the CLI assembled from the routine's private members before the method
existed; tests/golden/markov_pair_loss.json holds that value per backend, computed there by `case()` below.  Emulator and GPU."""
import json
import os

import numpy as np
import torch

from backend_util import host_device  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "markov_pair_loss.json")
B, G = 2, 8


def case(device):
    """A Markov routine around the smallest block, with shuffle_grid, after one statistics batch; and a pair batch of 2 on 8 x 8."""
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    torch.manual_seed(1234)
    conv = FNOFactorized2DBlock(modes=4, width=32, input_dim=3, n_layers=1, share_weight=True, factor=4, ff_weight_norm=True,
                                gain=0.1)
    routine = Grid2DMarkovExperiment(conv, n_steps=1, shuffle_grid=True, grid_size=(G,), max_accumulations=100).to(device)
    rs = np.random.RandomState(17)
    x = (rs.standard_normal((B, G, G, 1)) + 0.3).astype(np.float32)
    y = (x + 0.1 * rs.standard_normal((B, G, G, 1))).astype(np.float32)
    batch = {k: torch.from_numpy(v).to(device) for k, v in dict(x=x, y=y, dx=x - y, dy=y - x).items()}
    routine.train()
    assert routine.training_step(batch, epoch=0) is None      # the statistics epoch: the normaliser sees the batch, no step
    return routine, batch


def test_pair_loss_is_the_former_cli_valid_loss_to_the_bit(host_device):
    routine, batch = case(host_device)
    state = {k: v.clone() for k, v in routine.state_dict().items()}
    routine.eval()
    got = float(routine.pair_loss(batch).item())
    with open(GOLDEN) as f:
        want = float.fromhex(json.load(f)["cpu" if host_device == "cpu" else "gpu"])
    assert got == want, (got.hex(), want.hex())
    assert all(torch.equal(v, state[k]) for k, v in routine.state_dict().items())      # no step, no statistics
