#!/usr/bin/env python3
"""What the wide F-FNO block (widths 96 .. 256: fourierflow_amd/engine_wide.py over csrc/bgemm.hip) costs on the GPU: ms per
forward and per training step at widths 96 and 128, factor 4, 24 layers, 16 modes, batch 32, 64 x 64, against

  (a) the oracle block (oracle.ffno_oracle.ffno2d_block: eager torch.fft / einsum / linear, torch.optim.AdamW) run by torch on
      the same GPU at the same width -- the yardstick,
  (b) the width-64 engine (the tuned kernels) at the same geometry -- for scale only.

Every side gets warm-up calls, then --rounds rounds in which the sides alternate, each round long enough that a side collects
at least --seconds of timed work over the rounds; host clock around calls that end in a device synchronise; the median of the
rounds and their spread.  One JSON line; profiles/wide_engine.md holds a run.  From the repository root:  python tools/time_wide.py

  --mesh airfoil|plasticity   the wide MESH operators instead (WideFFNOMeshEngine; the pad / crop kernels of csrc/meshpad.hip):
                         airfoil     FNOFactorizedMesh2D, 221 x 51 (padded 229 x 59), batch 10, modes 32 / 16, 4 layers
                         plasticity  FNOFactorizedMesh3D, 101 x 31 x 20 (padded 109 x 39 x 28), batch 2, modes 32 / 12 / 8, 4 layers
                         at the reference configs' other hyper-parameters, against oracle.ffno_oracle.ffno_mesh2d / ffno_mesh3d;
                         no width-64 row.  profiles/wide_mesh.md holds a run.  Goes with --sites and --only as well.
  --sites --width W      per call site of one wide training step: launches, shape-derived FLOPs, device time (HIP events
                         around every launch) and the achieved TF/s against the 157 TF fp32 matrix peak; the same for one
                         forward-only pass with the fused feed-forward launch (`infer_sites`: wide_ff in place of wide_ff1 +
                         wide_ff2) and without it (`infer_pair_sites`)
  --only fwd|step --width W [--iters I] [--fuse-ff 0|1]   that side alone after a warm-up: what a `rocprofv3 --kernel-trace
                         --stats` run of its own is pointed at; --fuse-ff sets the engine's fuse_ff for the forward
  --infer                the forward-only pass with the fused feed-forward launch (csrc/bgemm_ff.hip, engine.fuse_ff = True) against
                         the same pass on the pair of launches (fuse_ff = False): ONE engine instance and one set of weights, the
                         two recorded passes alternating in this process, --rounds rounds, median and spread = max - min; also
                         whether the two outputs are equal bit for bit, and the workspace of each.  With --widths, and with --mesh.
                         profiles/wide_infer.md holds a run.
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
ap.add_argument("--mesh", choices=("airfoil", "plasticity"))
ap.add_argument("--sites", action="store_true")
ap.add_argument("--only", choices=("fwd", "step"))
ap.add_argument("--width", type=int, default=128)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--infer", action="store_true")
ap.add_argument("--fuse-ff", type=int, choices=(0, 1))
args = ap.parse_args()

import torch  # noqa: E402

from fourierflow_amd.modules import FNOFactorized2DBlock, FNOFactorizedMesh2D, FNOFactorizedMesh3D  # noqa: E402
from fourierflow_amd.trainer import FFNOTrainer  # noqa: E402
from oracle import ffno_oracle as orc  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("time_wide.py measures on the GPU: no device found")
dev = torch.device("cuda:0")
PEAK_TF = 157.0
MESH = dict(airfoil=dict(size=(221, 51), batch=10, modes=(32, 16), layers=4, output_dim=1),
            plasticity=dict(size=(101, 31, 20), batch=2, modes=(32, 12, 8), layers=4, output_dim=4))
mesh = MESH.get(args.mesh)
gen = torch.Generator().manual_seed(1)
if mesh:
    B, SIZE, nd = mesh["batch"], mesh["size"], len(mesh["size"])
    x = torch.randn(B, *SIZE, 1, generator=gen).to(dev)      # (the model appends one coordinate channel per axis)
    t = torch.randn(B, *SIZE, mesh["output_dim"], generator=gen).to(dev)
    shape = dict(mesh=args.mesh, batch=B, size=list(SIZE), padding=8, layers=mesh["layers"], modes=list(mesh["modes"]), factor=4)
else:
    B, G = args.batch, args.grid
    SIZE = (G, G)
    x = torch.randn(B, G, G, 3, generator=gen).to(dev)
    t = torch.randn(B, G, G, 1, generator=gen).to(dev)
    shape = dict(batch=B, grid=G, layers=args.layers, modes=args.modes, factor=args.factor)


def config(width):
    if mesh:      # experiments/airfoil/ffno/4_layers, experiments/plasticity/ffno/4_layers
        kw = dict(zip(("modes_x", "modes_y", "modes_z"), mesh["modes"]), width=width, input_dim=1 + nd, n_layers=mesh["layers"],
                  share_weight=False, factor=4, ff_weight_norm=True, n_ff_layers=2, layer_norm=False)
        return dict(kw, output_dim=mesh["output_dim"]) if nd == 3 else kw
    return dict(modes=args.modes, width=width, n_layers=args.layers, input_dim=3, share_weight=True, factor=args.factor,
                ff_weight_norm=True, gain=0.1)


def initial_state(width):
    """The reference-layout state dict both sides start from (shared tensors appear under every layer's key)."""
    if mesh:
        torch.manual_seed(0)
        return (FNOFactorizedMesh3D if nd == 3 else FNOFactorizedMesh2D)(**config(width)).state_dict()
    return orc.init_block_state_dict(**config(width), seed=0)


def oracle_model(sd, inp):
    if mesh:
        with torch.device(dev):      # (the oracle builds its coordinate channels on the default device, every call like the reference)
            return (orc.ffno_mesh3d if nd == 3 else orc.ffno_mesh2d)(sd, inp, modes=mesh["modes"], n_layers=mesh["layers"])
    return orc.ffno2d_block(sd, inp, modes=args.modes, n_layers=args.layers)["forecast"]


def engine_sides(width):
    """{side: callable} of our model at `width`: the inference forward and the full training step."""
    kw = config(width)
    blk = (FNOFactorizedMesh3D if nd == 3 else FNOFactorizedMesh2D)(**kw) if mesh else FNOFactorized2DBlock(**kw)
    blk.load_state_dict(initial_state(width))
    tr = FFNOTrainer(blk.to(dev))
    return tr, dict(fwd=lambda: tr.predict(x), step=lambda: tr.train_step(x, t))


def oracle_sides(width):
    sd, uniq, seen = {}, [], {}
    for k, v in initial_state(width).items():      # the shared Fourier weights appear under every layer's key
        if id(v) not in seen:
            seen[id(v)] = v.detach().to(dev).requires_grad_(True)
            uniq.append(seen[id(v)])
        sd[k] = seen[id(v)]
    opt = torch.optim.AdamW(uniq, lr=2.5e-3, weight_decay=1e-4)

    def fwd():
        with torch.no_grad():
            return oracle_model(sd, x)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = orc.lp_rel_loss(oracle_model(sd, x), t)
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


def set_fuse(eng, on):
    def run():
        eng.fuse_ff = on
        return tr.predict(x)
    return run


if args.infer:
    out = dict(shape=dict(shape, rounds=args.rounds, seconds=args.seconds), rows=[])
    for width in [int(w) for w in args.widths.split(",")]:
        tr, _ = engine_sides(width)
        eng = tr.engine
        sides = dict(fused=set_fuse(eng, True), pair=set_fuse(eng, False))
        y, recorded = {}, {}
        for name, fn in sides.items():
            y[name] = fn().clone()
            recorded[name] = sorted({o[0] for o in eng._last.fwd if o[0].startswith("wide_ff")})
        iters = {}
        for name, fn in sides.items():
            timed(fn, 2)
            iters[name] = max(1, int(args.seconds * 1e3 / args.rounds / timed(fn, 2)) + 1)
        rounds = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                rounds[name].append(timed(fn, iters[name]))
        row = dict(width=width, bit_identical=bool(torch.equal(y["fused"], y["pair"])), feed_forward_sites=recorded)
        for name, r in rounds.items():
            row[name] = dict(ms=round(statistics.median(r), 4), spread_ms=round(max(r) - min(r), 4), iters_per_round=iters[name],
                             rounds=[round(v, 4) for v in r],
                             workspace_bytes=eng.forward_workspace_bytes(B, *SIZE, fused=name == "fused"))
        gain = row["pair"]["ms"] - row["fused"]["ms"]
        row["pair_minus_fused_ms"] = round(gain, 4)
        row["pair_over_fused"] = round(row["pair"]["ms"] / row["fused"]["ms"], 4)
        # the rule of profiles/wide_infer.md: the fused median below the pair's by more than the larger of the two spreads
        row["fused_wins"] = bool(gain > max(row["fused"]["spread_ms"], row["pair"]["spread_ms"]))
        out["rows"].append(row)
        del tr, eng, sides
        torch.cuda.empty_cache()
    print(json.dumps(out))
    sys.exit(0)

if args.only:
    tr, sides = engine_sides(args.width)
    if args.fuse_ff is not None:
        tr.engine.fuse_ff = bool(args.fuse_ff)
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
    def site_rows(totals, flops):
        rows = []
        for name, (n, ms) in sorted(totals.items(), key=lambda kv: -kv[1][1]):
            tf = flops[name] / (ms * 1e-3) / 1e12 if name in flops and ms > 0 else None
            rows.append(dict(site=name, launches=n, ms=round(ms, 4), gflop=round(flops.get(name, 0) / 1e9, 3),
                             tf_per_s=None if tf is None else round(tf, 2), of_peak=None if tf is None else round(tf / PEAK_TF, 4)))
        return rows

    def infer_sites(fuse):
        """One forward-only pass, with or without the fused feed-forward launch."""
        run = set_fuse(eng, fuse)
        timed(run, 2)
        t = eng.timer = SiteTimer()
        run()
        eng.timer = None
        fl = {}
        for name, _fn, _args, keep in eng._last.fwd:
            d = keep[0] if keep else None
            if hasattr(d, "G0"):
                fl[name] = fl.get(name, 0) + 2.0 * d.M * d.N * d.K * d.G0 * d.G1
            elif hasattr(d, "W1"):      # the fused feed-forward descriptor: both products
                fl[name] = fl.get(name, 0) + 4.0 * d.P * d.C * d.H
        return site_rows(t.totals(), fl)

    rows = site_rows(totals, flops)
    print(json.dumps(dict(width=args.width, shape=shape,
                          step_device_ms=round(sum(ms for _, ms in totals.values()), 4), peak_tf=PEAK_TF, sites=rows,
                          infer_sites=infer_sites(True), infer_pair_sites=infer_sites(False),
                          workspace_bytes_per_layer=eng.workspace_bytes_per_layer(B, *SIZE),
                          forward_workspace_bytes=dict(fused=eng.forward_workspace_bytes(B, *SIZE, fused=True),
                                                       pair=eng.forward_workspace_bytes(B, *SIZE, fused=False)))))
    sys.exit(0)

out = dict(shape=dict(shape, rounds=args.rounds, seconds=args.seconds), rows=[])
for width in [int(w) for w in args.widths.split(",")] + ([] if mesh else [64]):
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
