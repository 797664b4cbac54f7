#!/usr/bin/env python3
"""What `train CONFIG --builder` costs for the two torus_li configs at the real shape of their dataset, on the GPU.  A synthetic
`u [1200, 64, 64, 20]` is written as a .mat file and read back by the builders (train 1000, test 200, ssr 1), then

  markov/24_layers (24 layers, width 64, 16 modes, noise 0.01; batch 19) through NSMarkovBuilder:
    statistics_epoch_s    the whole epoch 0: every training batch drawn and accumulated into the normaliser, no optimisation
    builder ms_per_step   optimisation steps of an epoch drawn from the builder's training set
    trajectory_file       the same steps from a MarkovTrajectoryData built as `train --data TRAJ.npz --epochs` builds it (the path
                          tools/time_data_path.py times at batch 32), alternating with the builder's within each repeat
    validation_s          `validation_step` over the whole validation split (200 trajectories: 11 batches of 10 model steps)
  zongyi/4_layers (FNOZongyi2DBlock 12 modes, width 20, 4 layers; 10-step rollout; batch 20) through NSZongyiBuilder:
    ms_per_step           optimisation steps of its epoch (50 at the real sizes), and validation_s as above

Medians of --repeats repeats of --steps steps.  One JSON line; profiles/torus_li_builder.md holds a run.  From the repository
root:  python tools/time_ns_builder.py"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import scipy.io
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fourierflow_amd.builders import MarkovTrajectoryData, NSMarkovBuilder, NSZongyiBuilder  # noqa: E402
from fourierflow_amd.cli import _split_loss  # noqa: E402
from fourierflow_amd.modules import FNOFactorized2DBlock, FNOZongyi2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment, Grid2DRolloutExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100, help="optimisation steps per repeat (Markov; the rollout routine runs up to one epoch)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--trajectories", type=int, default=1200)
ap.add_argument("--train-size", type=int, default=1000)
ap.add_argument("--test-size", type=int, default=200)
ap.add_argument("--layers", type=int, default=24)
args = ap.parse_args()

G, T = 64, 20
dev = torch.device("cuda:0")


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def cycle(data):
    while True:
        yield from data.epoch()


def median(values, digits=4):
    return dict(median=round(statistics.median(values), digits), repeats=[round(v, digits) for v in values])


with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "NavierStokes_V1e-5_N1200_T20.mat")
    scipy.io.savemat(path, {"u": np.random.RandomState(0).standard_normal((args.trajectories, G, G, T)).astype(np.float32)})
    t0 = time.perf_counter()
    markov = NSMarkovBuilder(path, args.train_size, args.test_size, 1, batch_size=19, num_workers=4, pin_memory=True)
    load_s = time.perf_counter() - t0
    zongyi = NSZongyiBuilder(path, args.train_size, args.test_size, 1, 10, batch_size=20, num_workers=4, pin_memory=True)
out = dict(shape=dict(trajectories=args.trajectories, train_size=args.train_size, test_size=args.test_size, grid=G, T=T,
                      layers=args.layers, steps=args.steps), load_mat_s=round(load_s, 2))

# -- markov/24_layers ------------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
conv = FNOFactorized2DBlock(modes=16, width=64, n_layers=args.layers, input_dim=3, share_weight=True, factor=4, ff_weight_norm=True,
                            gain=0.1)
exp = Grid2DMarkovExperiment(conv, n_steps=10, max_accumulations=1000, noise_std=0.01).to(dev)
train = markov.train_data(dev, seed=0)
from_file = MarkovTrajectoryData(markov.u[:args.train_size], device=dev, batch_size=19, mode="ns_markov", k=1, seed=0)
valid = markov.valid_data(dev)
t0 = sync_time()
for batch in train.epoch():
    exp.training_step(batch, epoch=0)
stats_s = sync_time() - t0
sources = dict(builder=cycle(train), trajectory_file=cycle(from_file))


def timed(it, steps):
    t0 = sync_time()
    for _ in range(steps):
        exp.training_step(next(it), epoch=1)
    return 1e3 * (sync_time() - t0) / steps


for it in sources.values():      # warm-up; also past max_accumulations = 1000 (948 batches so far), after which no step accumulates
    timed(it, 30)
rounds = {name: [] for name in sources}
for _ in range(args.repeats):
    for name, it in sources.items():
        rounds[name].append(timed(it, args.steps))
_split_loss(exp, valid)
valid_s = []
for _ in range(args.repeats):
    t0 = sync_time()
    metrics = _split_loss(exp, valid)
    valid_s.append(sync_time() - t0)
out["markov_24_layers"] = dict(batch=19, batches_per_epoch=len(train), statistics_epoch_s=round(stats_s, 3),
                               builder_ms_per_step=median(rounds["builder"]), trajectory_file_ms_per_step=median(rounds["trajectory_file"]),
                               builder_over_trajectory_file=round(statistics.median(rounds["builder"]) /
                                                                  statistics.median(rounds["trajectory_file"]), 4),
                               validation_s=median(valid_s), validation_batches=len(valid), valid_loss=round(metrics["valid_loss"], 4))
del exp, conv, train, from_file, valid, sources
torch.cuda.empty_cache()

# -- zongyi/4_layers -------------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
exp = Grid2DRolloutExperiment(FNOZongyi2DBlock(modes1=12, modes2=12, width=20, n_layers=4), n_steps=10).to(dev)
train, valid = zongyi.train_data(dev, seed=0), zongyi.valid_data(dev)
it = cycle(train)
steps = min(args.steps, len(train))
for _ in range(5):
    exp.training_step(next(it), 0)
ms = []
for _ in range(args.repeats):
    t0 = sync_time()
    for j in range(steps):
        exp.training_step(next(it), j)
    ms.append(1e3 * (sync_time() - t0) / steps)
_split_loss(exp, valid)
valid_s = []
for _ in range(args.repeats):
    t0 = sync_time()
    _split_loss(exp, valid)
    valid_s.append(sync_time() - t0)
out["zongyi_4_layers"] = dict(batch=20, batches_per_epoch=len(train), steps=steps, ms_per_step=median(ms), validation_s=median(valid_s),
                              validation_batches=len(valid))
print(json.dumps(out))
