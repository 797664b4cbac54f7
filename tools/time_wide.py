#!/usr/bin/env python3
"""What the wide F-FNO block (widths 96 .. 256: fourierflow_amd/engine_wide.py over csrc/bgemm.hip) costs on the GPU: ms per
forward and per training step at widths 96 and 128, factor 4, 24 layers, 16 modes, batch 32, 64 x 64, against

  (a) the oracle block (oracle.ffno_oracle.ffno2d_block: eager torch.fft / einsum / linear, torch.optim.AdamW) run by torch on
      the same GPU at the same width -- the yardstick,
  (b) the width-64 engine (the tuned kernels) at the same geometry -- for scale only.

Every side gets warm-up calls, then --rounds rounds in which the sides alternate, each round long enough that a side collects
at least --seconds of timed work over the rounds; host clock around calls that end in a device synchronise; the median of the
rounds and their spread.  One JSON line; profiles/wide_engine.md holds a run.  From the repository root:  python tools/time_wide.py

  --sites --width W      per call site of one wide training step: launches, shape-derived FLOPs, device time (HIP events
                         around every launch) and the achieved TF/s against the 157 TF fp32 matrix peak
  --only fwd|step --width W [--iters I]   that side alone after a warm-up: what a `rocprofv3 --kernel-trace --stats` run of its
                                          own is pointed at
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--widths", default="96,128")
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--modes", type=int, default=16)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--grid", type=int, default=64)
ap.add_argument("--factor", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--sites", action="store_true")
ap.add_argument("--only", choices=("fwd", "step"))
ap.add_argument("--width", type=int, default=128)
ap.add_argument("--iters", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402

from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.trainer import FFNOTrainer  # noqa: E402
from oracle import ffno_oracle as orc  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_wide.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
PEAK_TF = 157.0
B, G = args.batch, args.grid
gen = torch.Generator().manual_seed(1)
x = torch.randn(B, G, G, 3, generator=gen).to(dev)
t = torch.randn(B, G, G, 1, generator=gen).to(dev)


def config(width):
    return dict(modes=args.modes, width=width, n_layers=args.layers, input_dim=3, share_weight=True, factor=args.factor,
                ff_weight_norm=True, gain=0.1)


def engine_sides(width):
    """{side: callable} of our block at `width`: the inference forward and the full training step."""
    kw = config(width)
    sd = orc.init_block_state_dict(**kw, seed=0)
    blk = FNOFactorized2DBlock(**kw)
    blk.load_state_dict(sd)
    tr = FFNOTrainer(blk.to(dev))
    return tr, dict(fwd=lambda: tr.predict(x), step=lambda: tr.train_step(x, t))


def oracle_sides(width):
    kw = config(width)
    sd, uniq, seen = {}, [], {}
    for k, v in orc.init_block_state_dict(**kw, seed=0).items():      # the shared Fourier weights appear under every layer's key
        if id(v) not in seen:
            seen[id(v)] = v.to(dev).requires_grad_(True)
            uniq.append(seen[id(v)])
        sd[k] = seen[id(v)]
    opt = torch.optim.AdamW(uniq, lr=2.5e-3, weight_decay=1e-4)

    def fwd():
        with torch.no_grad():
            return orc.ffno2d_block(sd, x, modes=args.modes, n_layers=args.layers)["forecast"]

    def step():
        opt.zero_grad(set_to_none=True)
        loss = orc.lp_rel_loss(orc.ffno2d_block(sd, x, modes=args.modes, n_layers=args.layers)["forecast"], t)
        loss.backward()
        opt.step()
        return loss

    return dict(fwd=fwd, step=step)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


class SiteTimer:
    """The timer protocol of EngineCore._k: HIP events around every launch, summed per call-site name."""

    def __init__(self):
        self.events, self.open = {}, {}

    def want(self, name):
        return True

    def start(self, name, stream):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.open[name] = e

    def stop(self, name, stream):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.events.setdefault(name, []).append((self.open.pop(name), e))

    def totals(self):
        torch.cuda.synchronize()
        return {n: (len(ev), sum(a.elapsed_time(b) for a, b in ev)) for n, ev in self.events.items()}


if args.only:
    tr, sides = engine_sides(args.width)
    timed(sides[args.only], 2)
    print(json.dumps(dict(side=args.only, width=args.width, iters=args.iters, ms=round(timed(sides[args.only], args.iters), 4))))
    sys.exit(0)

if args.sites:
    tr, sides = engine_sides(args.width)
    timed(sides["step"], 2)
    eng = tr.engine
    timer = eng.timer = SiteTimer()
    sides["step"]()
    eng.timer = None
    totals = timer.totals()
    flops = {}
    ws = eng._last
    for name, _fn, _args, keep in ws.fwd + ws.bwd:      # the recorded pass: GEMM call sites keep their descriptor first
        d = keep[0] if keep and hasattr(keep[0], "G0") else None
        if d is not None:
            flops[name] = flops.get(name, 0) + 2.0 * d.M * d.N * d.K * d.G0 * d.G1
    rows = []
    for name, (n, ms) in sorted(totals.items(), key=lambda kv: -kv[1][1]):
        tf = flops[name] / (ms * 1e-3) / 1e12 if name in flops and ms > 0 else None
        rows.append(dict(site=name, launches=n, ms=round(ms, 4), gflop=round(flops.get(name, 0) / 1e9, 3),
                         tf_per_s=None if tf is None else round(tf, 2), of_peak=None if tf is None else round(tf / PEAK_TF, 4)))
    print(json.dumps(dict(width=args.width, shape=dict(batch=B, grid=G, layers=args.layers, modes=args.modes, factor=args.factor),
                          step_device_ms=round(sum(ms for _, ms in totals.values()), 4), peak_tf=PEAK_TF, sites=rows,
                          workspace_bytes_per_layer=eng.workspace_bytes_per_layer(B, G, G))))
    sys.exit(0)

out = dict(shape=dict(batch=B, grid=G, layers=args.layers, modes=args.modes, factor=args.factor, rounds=args.rounds,
                      seconds=args.seconds), rows=[])
for width in [int(w) for w in args.widths.split(",")] + [64]:
    tr, ours = engine_sides(width)
    sides = {f"engine_{k}": v for k, v in ours.items()}
    if width != 64:
        sides.update({f"oracle_{k}": v for k, v in oracle_sides(width).items()})
    iters = {}
    for name, fn in sides.items():      # warm-up, and the iterations one round needs
        timed(fn, 2)
        iters[name] = max(1, int(args.seconds * 1e3 / args.rounds / timed(fn, 2)) + 1)
    rounds = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            rounds[name].append(timed(fn, iters[name]))
    row = dict(width=width)
    for name, r in rounds.items():
        row[name] = dict(ms=round(statistics.median(r), 4), spread_ms=round(max(r) - min(r), 4), iters_per_round=iters[name],
                         rounds=[round(v, 4) for v in r])
    if width != 64:
        row["oracle_over_engine_fwd"] = round(row["oracle_fwd"]["ms"] / row["engine_fwd"]["ms"], 4)
        row["oracle_over_engine_step"] = round(row["oracle_step"]["ms"] / row["engine_step"]["ms"], 4)
    out["rows"].append(row)
    del tr, ours, sides
    torch.cuda.empty_cache()
print(json.dumps(out))
