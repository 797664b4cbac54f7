#!/usr/bin/env python3
"""What the training data path of the mesh routine costs per step on the GPU, and what one ffno_sample_gather launch takes.

1. ms per training step on the airfoil geometry (221 x 51, batch 10, FNOFactorizedMesh2D of --layers layers, width 64), with the
   batches coming from

  (a) npz:     an x / y file through `Batches` of builders/file_batches.py (a host slice and a synchronous copy per step, file order),
  (b) device:  the same samples through StructuredMesh2DBuilder -> DeviceSampleData (one ffno_sample_gather launch per step, a
               shuffled permutation per epoch),
  (c) fixed:   one batch that stays on the device,

   --repeats repeats of --steps steps each, the three sides alternating within a repeat; best and median of the repeats.

2. The gather launch alone: device events around --launches back-to-back `DeviceSampleData.gather` calls for the airfoil
   (batch 10), plasticity (101 x 31 x 20, batch 2) and elasticity (972 points, batch 20) batches, against torch producing the
   same tensors (`index_select` + `stack` / `expand` / `contiguous`).  Elasticity is measured from both source layouts: sample-major
   rows (transposed once at load, what ElasticityBuilder does) and the files' sample-axis-last layout (`src_sample = 1`).

One JSON line; profiles/sample_data_path.md holds a run.  From the repository root:  python tools/time_sample_data.py"""
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

from fourierflow_amd.builders import ElasticityBuilder, PlasticityBuilder, StructuredMesh2DBuilder  # noqa: E402
from fourierflow_amd.builders.sample_data import DeviceSampleData, Field  # noqa: E402
from fourierflow_amd.builders.file_batches import Batches  # noqa: E402
from fourierflow_amd.modules import FNOFactorizedMesh2D  # noqa: E402
from fourierflow_amd.routines import StructuredMeshExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50, help="training steps per repeat")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--launches", type=int, default=1000, help="gather launches between the two device events")
ap.add_argument("--samples", type=int, default=200, help="samples in each training set")
ap.add_argument("--layers", type=int, default=4)
args = ap.parse_args()

dev = torch.device("cuda:0")
rs = np.random.RandomState(0)
n = args.samples
X, Y, B = 221, 51, 10
out = dict(shape=dict(mesh=[X, Y], batch=B, samples=n, layers=args.layers, steps=args.steps, launches=args.launches))


def events(fn, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for j in range(count):
        fn(j)
    stop.record()
    torch.cuda.synchronize()
    return 1e3 * start.elapsed_time(stop) / count


def launch_us(fn):
    for j in range(10):
        fn(j)
    r = [events(fn, args.launches) for _ in range(args.repeats)]
    return dict(best=round(min(r), 3), median=round(statistics.median(r), 3), repeats=[round(v, 3) for v in r])


def perm(m):
    return torch.randperm(m, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)


with tempfile.TemporaryDirectory() as tmp:
    # ---- 1. the training step ------------------------------------------------------------------------------------
    x1, x2 = rs.standard_normal((n, X, Y)), rs.standard_normal((n, X, Y))
    q = rs.standard_normal((n, 5, X, Y))
    for name, a in (("X", x1), ("Y", x2), ("Q", q)):
        np.save(os.path.join(tmp, name + ".npy"), a)
    airfoil = StructuredMesh2DBuilder(os.path.join(tmp, "X.npy"), os.path.join(tmp, "Y.npy"), os.path.join(tmp, "Q.npy"), 4, n, 0, 0,
                                      batch_size=B)
    np.savez(os.path.join(tmp, "train.npz"), x=np.stack([x1, x2], -1).astype(np.float32), y=q[:, 4, :, :, None].astype(np.float32))
    torch.manual_seed(0)
    exp = StructuredMeshExperiment(FNOFactorizedMesh2D(modes_x=32, modes_y=16, width=64, input_dim=4, n_layers=args.layers,
                                                       share_weight=False, factor=4, ff_weight_norm=True, n_ff_layers=2,
                                                       layer_norm=False)).to(dev)
    npz = Batches(exp, {}, dev, os.path.join(tmp, "train.npz"), B, 64, None, seed=0)
    device_set = airfoil.train_data(dev, seed=0)
    fixed = next(iter(airfoil.train_data(dev, seed=0)))

    def forever(batch):
        while True:
            yield batch

    sources = dict(npz=iter(npz), device=iter(device_set), fixed=forever(fixed))

    def timed(it, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            exp.training_step(next(it))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    for it in sources.values():
        timed(it, 10)
    rounds = {name: [] for name in sources}
    for _ in range(args.repeats):
        for name, it in sources.items():
            rounds[name].append(timed(it, args.steps))
    for name, r in rounds.items():
        out[name] = dict(ms_per_step_best=round(min(r), 4), ms_per_step_median=round(statistics.median(r), 4),
                         spread_ms=round(max(r) - min(r), 4), repeats=[round(v, 4) for v in r])
    out["device_minus_npz_ms_best"] = round(out["device"]["ms_per_step_best"] - out["npz"]["ms_per_step_best"], 4)

    # ---- 2. the launch alone --------------------------------------------------------------------------------------
    ids = perm(n)
    tx1, tx2, ty = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (x1, x2, q[:, 4]))

    def torch_airfoil(j):
        i = ids[(j * B) % (n - B + 1):][:B]
        return dict(x=torch.stack([tx1.index_select(0, i), tx2.index_select(0, i)], -1), y=ty.index_select(0, i).unsqueeze(-1))

    out["airfoil"] = dict(gather_us=launch_us(lambda j: device_set.gather(ids, (j * B) % (n - B + 1), B)), torch_us=launch_us(torch_airfoil))

    s1, s2, t, Bp, npl = 101, 31, 20, 2, min(n, 64)
    inp, outp = rs.standard_normal((npl, s1)), rs.standard_normal((npl, s1, s2, t, 4)).astype(np.float32)
    scipy.io.savemat(os.path.join(tmp, "plas.mat"), dict(input=inp, output=outp))
    plas = PlasticityBuilder(os.path.join(tmp, "plas.mat"), npl, 0, 0, s1, s2, t, batch_size=Bp).train_data(dev, seed=0)
    pids = perm(npl)
    tin, tout = torch.from_numpy(inp.astype(np.float32)).to(dev), torch.from_numpy(outp).to(dev)

    def torch_plasticity(j):
        i = pids[(j * Bp) % (npl - Bp + 1):][:Bp]
        return dict(x=tin.index_select(0, i)[:, :, None, None, None].expand(Bp, s1, s2, t, 1).contiguous(), y=tout.index_select(0, i))

    out["plasticity"] = dict(samples=npl, batch=Bp, gather_us=launch_us(lambda j: plas.gather(pids, (j * Bp) % (npl - Bp + 1), Bp)),
                             torch_us=launch_us(torch_plasticity))

    P, Be = 972, 20
    rr, sigma, xy = rs.standard_normal((42, n)), rs.standard_normal((P, n)), rs.uniform(0, 1, (P, 2, n))
    for name, a in (("rr", rr), ("sigma", sigma), ("xy", xy)):
        np.save(os.path.join(tmp, name + ".npy"), a)
    rows_set = ElasticityBuilder(os.path.join(tmp, "sigma.npy"), os.path.join(tmp, "xy.npy"), os.path.join(tmp, "rr.npy"), n, 0, 0,
                                 batch_size=Be).train_data(dev, seed=0)
    file_set = DeviceSampleData([Field("xy", xy, (P, 2), P, 2, (1, 0, 2 * n, n), (0, 2, 1)),
                                 Field("rr", rr, (42,), 1, 42, (1, 0, 0, n), (0, 0, 1)),
                                 Field("sigma", sigma, (P, 1), 1, P, (1, 0, 0, n), (0, 0, 1))], n, device=dev, batch_size=Be, seed=0)
    a, b = rows_set.gather(ids, 3, Be), file_set.gather(ids, 3, Be)
    assert all(torch.equal(a[k], b[k]) for k in a)
    txy, trr, tsg = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
                     for v in (np.transpose(xy, (2, 0, 1)), rr.T, sigma.T[..., None]))

    def torch_elasticity(j):
        i = ids[(j * Be) % (n - Be + 1):][:Be]
        return dict(xy=txy.index_select(0, i), rr=trr.index_select(0, i), sigma=tsg.index_select(0, i))

    out["elasticity"] = dict(batch=Be, points=P,
                             gather_rows_us=launch_us(lambda j: rows_set.gather(ids, (j * Be) % (n - Be + 1), Be)),
                             gather_file_layout_us=launch_us(lambda j: file_set.gather(ids, (j * Be) % (n - Be + 1), Be)),
                             torch_us=launch_us(torch_elasticity))
print(json.dumps(out))
