#!/usr/bin/env python3
"""What a training step of a multi-resolution run costs on the GPU: the Markov routine of the torus_kochkov/ffno/multi_resolution
configs (24 layers, width 64, 16 modes, use_velocity: five input channels), batch 32, with the batches coming from

  single sizes    MarkovTrajectoryData at 32 x 32, 64 x 64 and 128 x 128: the geometry never changes,
  alternations    MultiResolutionMarkovData over 32/64, 32/128 and 64/128 with --num-workers loader workers (default 1: the geometry
                  changes at every step; the shipped configs say 4: four steps of one size, four of the other),

as the median of --repeats repeats of --steps steps each, all sides (or those of --only) alternating within a repeat, one routine
(one engine, one workspace per geometry) serving them all.  The sets hold 16 trajectories of T = 14 with k = 2: 192 pairs, six full batches per epoch,
so an alternation takes as many steps at one size as at the other and the expectation for it is the mean of its two sizes.  Also the
draw launch alone at each size (device events around --launches back-to-back launches, so dispatch included), and the loss of the
last step of every window (the sides train ONE model, one after the other: the windows are not independent runs).  One JSON line;
profiles/multi_resolution.md holds a run.  From the repository root:  python tools/time_multi_resolution.py"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fourierflow_amd.builders.markov_data import MarkovTrajectoryData, MultiResolutionMarkovData  # noqa: E402
from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=96, help="training steps per repeat and side (a multiple of 2 x num-workers)")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=500, help="draw launches between the two device events")
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--num-workers", type=int, default=1)
ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128])
ap.add_argument("--only", nargs="+", default=None, help="the sides to run, e.g. 32/128 or 32 128 (a kernel trace of one side: "
                                                        "rocprofv3 --kernel-trace --stats -- python tools/time_multi_resolution.py "
                                                        "--only 32/128); default: all")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/time_multi_resolution.py measures on an MI355X: no GPU here")
if args.steps % (2 * max(1, args.num_workers)):
    raise SystemExit("--steps must be a multiple of 2 x --num-workers, so that an alternation spends half its steps at each size")

B, N_TRAJ, T, K = 32, 16, 14, 2
dev = torch.device("cuda:0")
KW = dict(modes=16, width=64, n_layers=args.layers, input_dim=5, share_weight=True, factor=4, ff_weight_norm=True, gain=0.1)
torch.manual_seed(0)
exp = Grid2DMarkovExperiment(FNOFactorized2DBlock(**KW), use_velocity=True, grid_size=list(args.sizes), noise_std=0.01).to(dev)

rs = np.random.RandomState(0)
arrays = {g: rs.standard_normal((N_TRAJ, g, g, T)).astype(np.float32) for g in args.sizes}
singles = {g: MarkovTrajectoryData(arrays[g], device=dev, batch_size=B, mode="kolmogorov", k=K, seed=0) for g in args.sizes}
pairs = [(a, b) for i, a in enumerate(args.sizes) for b in args.sizes[i + 1:]]
# (the finer grid first, as in the shipped configs)
multis = {f"{a}/{b}": MultiResolutionMarkovData([arrays[b], arrays[a]], device=dev, batch_size=B, k=K, num_workers=args.num_workers,
                                                seed=0) for a, b in pairs}
sources = {**{str(g): iter(s) for g, s in singles.items()}, **{name: iter(m) for name, m in multis.items()}}
if args.only:
    unknown = [name for name in args.only if name not in sources]
    if unknown:
        raise SystemExit(f"--only {' '.join(unknown)}: the sides are {' '.join(sources)}")

for g in args.sizes:      # epoch 0: the normaliser statistics, every size
    for _ in range(2):
        exp.training_step(next(sources[str(g)]), epoch=0)
sources = {name: it for name, it in sources.items() if not args.only or name in args.only}


def timed(it, steps):
    """ms per step of a burst, and the loss of its last step (read after the clock has stopped)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = exp.training_step(next(it), epoch=1)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, float(loss.item())


for it in sources.values():      # every geometry of the timed windows, warm
    timed(it, 12)
cache = dict(exp.trainer().engine._ws_cache)
rounds, last_loss = {name: [] for name in sources}, {name: [] for name in sources}
for _ in range(args.repeats):
    for name, it in sources.items():
        ms, loss = timed(it, args.steps)
        rounds[name].append(ms)
        last_loss[name].append(loss)
after = exp.trainer().engine._ws_cache
workspaces_kept = set(after) == set(cache) and all(after[k] is cache[k] for k in cache)

launch_us = {}
for g, s in singles.items():
    if str(g) not in sources:
        continue
    ids = torch.randperm(s.n_pairs, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    for _ in range(10):
        s.gather(ids, 0, B)
    reps = []
    for _ in range(args.repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for j in range(args.launches):
            s.gather(ids, (j * B) % (s.n_pairs - B + 1), B)
        stop.record()
        torch.cuda.synchronize()
        reps.append(1e3 * start.elapsed_time(stop) / args.launches)
    launch_us[str(g)] = dict(median=round(statistics.median(reps), 3), repeats=[round(v, 3) for v in reps])

out = dict(shape=dict(batch=B, sizes=args.sizes, T=T, k=K, trajectories=N_TRAJ, layers=args.layers, steps=args.steps,
                      num_workers=args.num_workers), workspaces=len(cache), workspaces_kept=workspaces_kept)
for name, r in rounds.items():
    out[name] = dict(ms_per_step=round(statistics.median(r), 4), spread_ms=round(max(r) - min(r), 4), repeats=[round(v, 4) for v in r],
                     last_loss=[round(v, 4) for v in last_loss[name]])
for a, b in pairs:
    name = f"{a}/{b}"
    if not {str(a), str(b), name} <= set(rounds):
        continue
    mean = 0.5 * (out[str(a)]["ms_per_step"] + out[str(b)]["ms_per_step"])
    out[name].update(mean_of_sizes_ms=round(mean, 4), minus_mean_ms=round(out[name]["ms_per_step"] - mean, 4),
                     session_spread_ms=round(max(out[k]["spread_ms"] for k in (str(a), str(b), name)), 4))
out["draw_launch_us"] = launch_us
print(json.dumps(out))
