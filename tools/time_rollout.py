#!/usr/bin/env python3
"""What one step of an autoregressive rollout of the Markov routine costs on the GPU (markov/24: 24 layers, width 64, 16 modes,
64 x 64), through

  (a) rollout():   the feature launches, the engine, three or four torch element-wise kernels and a final torch.cat,
  (b) simulate():  the engine and one ffno_markov_advance launch per step,

at batch 1, 8 and 32, and with `use_velocity` at batch 1 (where simulate() fuses less: the velocity and feature launches stay).
Per row: --repeats repeats of --steps steps each after a warm-up call of both paths, the two paths alternating within a repeat,
host clock around a call that ends in a device synchronise; the median of the repeats.  One JSON line; profiles/markov_rollout.md
holds a run.  From the repository root:  python tools/time_rollout.py

  --only rollout|simulate --batch B [--velocity] --steps S   one call of one path after a warm-up call: what a
                                                             `rocprofv3 --kernel-trace` run of its own is pointed at
  --launches TRACE.csv                                       the launches of one step from that run's kernel-trace CSV: what lies
                                                             between the last two head launches, in start order (no GPU needed)
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=400, help="rollout steps per repeat")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--only", choices=("rollout", "simulate"))
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--velocity", action="store_true")
ap.add_argument("--launches", metavar="TRACE.csv")
args = ap.parse_args()


def short(name):
    """A kernel name without its argument list and with its template arguments cut to what tells two torch kernels apart."""
    name = re.sub(r"^void ", "", name.strip()).split("(")[0]
    op = re.search(r"(\w+Functor|\w+_kernel_cuda|CatArrayBatchedCopy\w*|direct_copy_kernel\w*)", name.split("<", 1)[1]) if "<" in name else None
    return name.split("<")[0] + (f"<{op.group(1)}>" if op else "")


if args.launches:
    with open(args.launches, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    heads = [i for i, n in enumerate(names) if "head_fwd" in n]
    if len(heads) < 3:
        raise SystemExit("the trace holds fewer than three head launches: run more steps")
    step = range(heads[-2] + 1, heads[-1] + 1)      # from the feedback of step n - 2 to the head of step n - 1
    print(f"{len(step)} launches per step ({len(names)} dispatches in the trace, {len(heads)} head launches); after the last head: "
          f"{', '.join(names[heads[-1] + 1:]) or 'nothing'}\n")
    print("| # | kernel | us |")
    print("|---|---|---|")
    for k, i in enumerate(step):
        print(f"| {k + 1} | `{names[i]}` | {(int(rows[i]['End_Timestamp']) - int(rows[i]['Start_Timestamp'])) / 1e3:.1f} |")
    sys.exit(0)

import torch  # noqa: E402

from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_rollout.py measures on the GPU: no device found")
G = 64
dev = torch.device("cuda:0")


def routine(velocity):
    kw = dict(modes=16, width=64, n_layers=args.layers, input_dim=5 if velocity else 3, share_weight=True, factor=4,
              ff_weight_norm=True, gain=0.1)
    torch.manual_seed(0)
    exp = Grid2DMarkovExperiment(FNOFactorized2DBlock(**kw), use_velocity=velocity, grid_size=[G]).to(dev)
    gen = torch.Generator().manual_seed(1)
    for _ in range(4):      # epoch 0: the normaliser statistics
        exp.training_step({"x": torch.randn(32, G, G, 1, generator=gen).to(dev)}, epoch=0)
    exp.eval()
    return exp


def timed(fn, x0, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(x0, steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, out


def x0_of(batch):
    return torch.randn(batch, G, G, 1, generator=torch.Generator().manual_seed(2)).to(dev)


if args.only:
    exp = routine(args.velocity)
    fn = getattr(exp, args.only)
    timed(fn, x0_of(args.batch), 3)
    ms, _ = timed(fn, x0_of(args.batch), args.steps)
    print(json.dumps(dict(path=args.only, batch=args.batch, use_velocity=args.velocity, steps=args.steps, ms_per_step=round(ms, 4))))
    sys.exit(0)

out = dict(shape=dict(grid=G, layers=args.layers, width=64, modes=16, steps=args.steps, repeats=args.repeats), rows=[])
for velocity, batches in ((False, (1, 8, 32)), (True, (1,))):
    exp = routine(velocity)
    for batch in batches:
        x0 = x0_of(batch)
        paths = dict(rollout=exp.rollout, simulate=exp.simulate)
        last = {}
        for name, fn in paths.items():
            timed(fn, x0, 20)
        rounds = {name: [] for name in paths}
        for _ in range(args.repeats):
            for name, fn in paths.items():
                ms, last[name] = timed(fn, x0, args.steps)
                rounds[name].append(ms)
        a, b = last["rollout"].double(), last["simulate"].double()
        k = min(10, args.steps)      # the two paths round the inverse affine differently: compared over the first steps only
        row = dict(batch=batch, use_velocity=velocity,
                   first_steps_rel_l2=float((a[..., :k] - b[..., :k]).norm() / b[..., :k].norm()),
                   finite=bool(torch.isfinite(last["simulate"][..., -1]).all()))
        for name, r in rounds.items():
            row[name] = dict(ms_per_step=round(statistics.median(r), 4), spread_ms=round(max(r) - min(r), 4),
                             repeats=[round(v, 4) for v in r])
        row["simulate_minus_rollout_ms"] = round(row["simulate"]["ms_per_step"] - row["rollout"]["ms_per_step"], 4)
        row["rollout_over_simulate"] = round(row["rollout"]["ms_per_step"] / row["simulate"]["ms_per_step"], 4)
        out["rows"].append(row)
        del last
print(json.dumps(out))
