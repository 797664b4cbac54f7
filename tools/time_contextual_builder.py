#!/usr/bin/env python3
"""What `train CONFIG --builder` costs per optimisation step for the torus_vis_force configs at the shape of their dataset, on
the GPU: 64 x 64 fields (256 x 256 after ssr = 4; written here at 64 x 64 and read with ssr = 1), T = 200 snapshots, k = 10,
batch 19, the 24-layer F-FNO of 01_baseline with the force and the viscosity appended (input_dim 5, noise 0.01).  Synthetic
trajectories are written as the three .npz files NSContextualBuilder reads, once with one force map per trajectory and once with
one per snapshot, then

  builder_const / builder_step   ms per training step with batches drawn from the builder's training set (one
                                 ffno_markov_pairs_tf launch per step, a shuffled permutation per epoch)
  fixed                          ms per training step on one batch that stays on the device (the floor `bench.py` measures)
  draw_launch_us                 one draw launch alone for either layout (device events around --launches back-to-back launches,
                                 so dispatch included)

as the median of --repeats repeats of --steps steps each, the three sides alternating within a repeat.  One JSON line;
profiles/contextual_builder.md holds a run.  From the repository root:  python tools/time_contextual_builder.py"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fourierflow_amd.builders import NSContextualBuilder  # noqa: E402
from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100, help="training steps per repeat")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=1000, help="draw launches between the two device events")
ap.add_argument("--trajectories", type=int, default=32, help="trajectories in the training file")
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--snapshots", type=int, default=200)
args = ap.parse_args()

B, G, T, K = 19, 64, args.snapshots, 10
dev = torch.device("cuda:0")
torch.manual_seed(0)
conv = FNOFactorized2DBlock(modes=16, width=64, n_layers=args.layers, input_dim=5, share_weight=True, factor=4, ff_weight_norm=True,
                            gain=0.1)
exp = Grid2DMarkovExperiment(conv, n_steps=10, max_accumulations=10000, noise_std=0.01, append_force=True, append_mu=True).to(dev)

rs = np.random.RandomState(0)
u = rs.standard_normal((args.trajectories, G, G, T)).astype(np.float32)
mu = rs.uniform(1e-5, 1e-4, args.trajectories).astype(np.float32)
forces = dict(const=rs.standard_normal((args.trajectories, G, G)).astype(np.float32),
              step=rs.standard_normal((args.trajectories, G, G, T)).astype(np.float32))
sets, load_s = {}, {}
with tempfile.TemporaryDirectory() as tmp:
    for layout, f in forces.items():
        prefix = os.path.join(tmp, f"torus_{layout}")
        np.savez(prefix + ".train.npz", data=u, f=f, mu=mu)
        for split in ("valid", "test"):      # the builder wants all three; two trajectories each
            np.savez(f"{prefix}.{split}.npz", data=u[:2], f=f[:2], mu=mu[:2])
        t0 = time.perf_counter()
        bld = NSContextualBuilder(prefix + ".h5", 1, K, batch_size=B, num_workers=16, pin_memory=True)
        sets[layout] = bld.train_data(dev, seed=0)
        load_s[layout] = round(time.perf_counter() - t0, 2)
del u, forces


def cycle(data):
    while True:
        yield from data.epoch()


def forever(batch):
    while True:
        yield batch


sources = dict(builder_const=cycle(sets["const"]), builder_step=cycle(sets["step"]),
               fixed=forever(next(sets["const"].epoch())))
for _ in range(4):      # epoch 0: the normaliser statistics
    exp.training_step(next(sources["builder_const"]), epoch=0)


def timed(it, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        exp.training_step(next(it), epoch=1)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


for it in sources.values():
    timed(it, 10)
rounds = {name: [] for name in sources}
for _ in range(args.repeats):
    for name, it in sources.items():
        rounds[name].append(timed(it, args.steps))

launch_us = {}
for layout, ds in sets.items():
    ids = torch.randperm(ds.n_pairs, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    for _ in range(10):
        ds.gather(ids, 0, B)
    launch_us[layout] = []
    for _ in range(args.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for j in range(args.launches):
            ds.gather(ids, (j * B) % (ds.n_pairs - B + 1), B)
        stop.record()
        torch.cuda.synchronize()
        launch_us[layout].append(1e3 * start.elapsed_time(stop) / args.launches)

out = dict(shape=dict(batch=B, grid=G, T=T, k=K, trajectories=args.trajectories, pairs=sets["const"].n_pairs,
                      batches_per_epoch=len(sets["const"]), layers=args.layers, steps=args.steps), load_and_upload_s=load_s)
for name, r in rounds.items():
    out[name] = dict(ms_per_step=round(statistics.median(r), 4), spread_ms=round(max(r) - min(r), 4), repeats=[round(v, 4) for v in r])
for name in ("builder_const", "builder_step"):
    out[name + "_over_fixed"] = round(out[name]["ms_per_step"] / out["fixed"]["ms_per_step"], 4)
out["draw_launch_us"] = {layout: dict(median=round(statistics.median(v), 3), repeats=[round(x, 3) for x in v])
                         for layout, v in launch_us.items()}
print(json.dumps(out))
