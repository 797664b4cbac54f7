#!/usr/bin/env python3
"""What the prediction export behind `pred_path` costs in the test of a torus_kochkov routine (24 layers, width 64, use_velocity,
10 steps; the batch sizes and modes of the three torus_kochkov/ffno/predictions configs: 32 / 32 / 12 at 64 / 128 / 256) on the
GPU, pred_size 64.  Writes profiles/pred_export.md (or --output) and prints one JSON line per measurement.

  batch     ms per test batch (`test_step`) of the routine with and without a pred_path; median of 5 rounds, the two sides alternating
  export    ffno_prediction_export_step alone against the same arithmetic written with torch ops on the device (strided slices, two
            means, two rolls, three copies into the slab); the largest difference between the two results goes along
  spectrum  ffno_energy_spectrum alone (on ready half spectra) against torch ops (squares, weights, index_add_ over precomputed
            shell indices); the largest relative difference goes along
  calls     the C-ABI calls of one test batch by entry point, and of one rollout step, with and without the export

Run from the repository root:  python tools/time_pred_export.py"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_reduced_corr import alternate, count_calls  # noqa: E402

from fourierflow_amd import _capi, _lib  # noqa: E402
from fourierflow_amd._lib import ptr as _p  # noqa: E402
from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment  # noqa: E402

CASES = ((64, 32, 16, 10), (128, 32, 32, 5), (256, 12, 32, 3))      # grid, batch, modes, test batches per round
N, T, PRED = 10, 11, 64
dev = "cuda:0"
TWO_PI = 2 * math.pi


def routine(G, B, modes, **kw):
    torch.manual_seed(0)
    conv = FNOFactorized2DBlock(modes=modes, width=64, n_layers=24, input_dim=5, share_weight=True, factor=4, ff_weight_norm=True,
                                gain=0.1)
    exp = Grid2DMarkovExperiment(conv, use_velocity=True, grid_size=[G], step_size=0.28, **kw).to(dev)
    for _ in range(2):
        exp.training_step(dict(x=torch.randn(B, G, G, 1, device=dev), y=torch.randn(B, G, G, 1, device=dev)), epoch=0)
    return exp.eval()


def torch_export(vel, slabs, t, m):
    """The arithmetic of ffno_prediction_export_step with torch ops, into slab t of slabs [3][n_steps][B][m][m]."""
    Bv, X, _, _ = vel.shape
    f = X // m
    if f == 1:
        slabs[:, t] = vel.permute(3, 0, 1, 2)
        return
    u_c = vel[:, f - 1::f, :, 1].reshape(Bv, m, m, f).mean(-1)
    v_c = vel[:, :, f - 1::f, 2].reshape(Bv, m, f, m).mean(2)
    slabs[0, t] = (torch.roll(v_c, -1, 1) - v_c) / (TWO_PI / m) - (torch.roll(u_c, -1, 2) - u_c) / (TWO_PI / m)
    slabs[1, t] = u_c
    slabs[2, t] = v_c


def shell_tables(m):
    r, c = np.meshgrid(np.arange(m), np.arange(m // 2 + 1), indexing="ij")
    kx = np.where(r < m // 2, r, r - m)
    s = np.floor(np.sqrt(kx * kx + c * c) + 0.5).astype(np.int64)      # (tests/test_kernels_energy_spectrum.py: equal to the integer rule)
    h = np.where((c == 0) | (c == m // 2), 1.0, 2.0).astype(np.float32) / (2.0 * float(m) ** 4)
    return torch.from_numpy(s.reshape(-1)).to(dev), torch.from_numpy(h.reshape(-1)).to(dev), int(s.max()) + 1


def torch_spectrum(spec, shells, weights, n_shells, m):
    """The arithmetic of ffno_energy_spectrum with torch ops: spec [2][n_img][m][m/2+1][2] -> E [n_img][m/2+1]."""
    e = (spec * spec).sum(-1).sum(0).reshape(spec.shape[1], -1) * weights
    return torch.zeros(spec.shape[1], n_shells, device=spec.device).index_add_(1, shells, e)[:, :m // 2 + 1]


def main(output):
    lib = _lib.get_lib()
    stream = _lib.current_stream(torch.device(dev))
    rows = {"batch": [], "export": [], "calls": []}
    for G, B, modes, reps in CASES:
        on, off = routine(G, B, modes, pred_path="preds.nc", pred_size=PRED), routine(G, B, modes)
        batch = dict(data=torch.randn(B, G, G, T, device=dev))
        t_off, t_on, r_off, r_on = alternate(lambda: off.test_step(batch), lambda: on.test_step(batch), reps)
        rows["batch"].append(dict(what="batch", grid=G, batch=B, modes=modes, n_steps=N, without_ms=t_off, with_ms=t_on,
                                  rounds_without=r_off, rounds_with=r_on))
        c_on, c_off = count_calls(lambda: on.test_step(batch)), count_calls(lambda: off.test_step(batch))
        rows["calls"].append(dict(what="calls", grid=G, with_export=c_on, without=c_off))
        del on, off
        vel = torch.randn(B, G, G, 3, device=dev)
        slabs, slabs_t = torch.zeros(3, N, B, PRED, PRED, device=dev), torch.zeros(3, N, B, PRED, PRED, device=dev)

        def kernel():
            _capi.check(lib.ffno_prediction_export_step(_p(vel), _p(slabs[0]), _p(slabs[1]), _p(slabs[2]), B, G, G, PRED, N, 3,
                                                        TWO_PI, TWO_PI, stream), "prediction_export_step")

        t_k, t_e, r_k, r_e = alternate(kernel, lambda: torch_export(vel, slabs_t, 3, PRED), 200)
        rows["export"].append(dict(what="export", grid=G, batch=B, pred_size=PRED, kernel_us=1e3 * t_k, torch_ops_us=1e3 * t_e,
                                   rounds_kernel=r_k, rounds_torch=r_e, max_abs_diff=float((slabs - slabs_t).abs().max())))
        for k in ("batch", "calls", "export"):
            print(json.dumps(rows[k][-1]), flush=True)
    rows["spectrum"] = []
    shells, weights, n_shells = shell_tables(PRED)
    for B in (32, 12):
        both = torch.randn(2, N, B, PRED, PRED, device=dev)
        spec = torch.view_as_real(torch.fft.rfft2(both)).contiguous().view(2, N * B, PRED, PRED // 2 + 1, 2)
        E = torch.empty(N * B, PRED // 2 + 1, device=dev)

        def kernel():
            _capi.check(lib.ffno_energy_spectrum(_p(spec[0]), _p(spec[1]), _p(E), N * B, PRED, stream), "energy_spectrum")

        t_k, t_e, r_k, r_e = alternate(kernel, lambda: torch_spectrum(spec, shells, weights, n_shells, PRED), 200)
        t_f = alternate(lambda: torch.fft.rfft2(both), lambda: torch.fft.rfft2(both), 200)[0]
        want = torch_spectrum(spec, shells, weights, n_shells, PRED)
        rows["spectrum"].append(dict(what="spectrum", images=N * B, pred_size=PRED, kernel_us=1e3 * t_k, torch_ops_us=1e3 * t_e,
                                     rfft2_us=1e3 * t_f, rounds_kernel=r_k, rounds_torch=r_e,
                                     max_rel_diff=float(((E - want).abs() / want).max())))
        print(json.dumps(rows["spectrum"][-1]), flush=True)
    write_report(output, rows)


def write_report(output, rows):
    spread = lambda r: ", ".join(f"{x:.3f}" for x in r)      # noqa: E731
    L = ["# What the prediction export behind `pred_path` costs in the test of a torus_kochkov routine on an MI355X", "",
         "`python tools/time_pred_export.py`, one session on one box.  The model of the `torus_kochkov/ffno/predictions` configs: 24 layers,",
         "width 64, 16 / 32 / 32 modes and batches of 32 / 32 / 12 at 64 / 128 / 256, shared Fourier weights, `use_velocity`; 10 rollout",
         "steps; `pred_size` 64; fp32; random N(0, 1) trajectories, weights as initialised (the timings do not depend on the values).",
         "Host clock around bursts that end in a device synchronise; the two sides of every comparison alternate within each round;",
         "medians of 5 rounds.  No threshold is set on any of these numbers.", "",
         "## One test batch (`test_step`)", "",
         "| grid | batch | without `pred_path`, ms | with, ms | difference | rounds (without / with) |", "|---|---|---|---|---|---|"]
    for r in rows["batch"]:
        d = r["with_ms"] - r["without_ms"]
        L.append(f"| {r['grid']} x {r['grid']} | {r['batch']} | **{r['without_ms']:.3f}** | **{r['with_ms']:.3f}** | "
                 f"{d:+.3f} ms ({100 * d / r['without_ms']:+.2f} %) | {spread(r['rounds_without'])} / {spread(r['rounds_with'])} |")
    L += ["", "With `use_velocity` the velocity image of step t's prediction is the one step t + 1's features need, so the export adds ONE",
          "`ffno_velocity_features` call per batch (the last step's), ten `ffno_prediction_export_step` launches, one batched `rfft2` and one",
          "`ffno_energy_spectrum` launch.", "",
          "## `ffno_prediction_export_step` alone (200 calls per round)", "",
          "| grid -> 64 | batch | kernel, us | torch ops, us | largest difference of the results | rounds (kernel / torch) |", "|---|---|---|---|---|---|"]
    for r in rows["export"]:
        L.append(f"| {r['grid']} | {r['batch']} | **{r['kernel_us']:.2f}** | {r['torch_ops_us']:.2f} | {r['max_abs_diff']:.2e} | "
                 f"{spread(1e3 * x for x in r['rounds_kernel'])} / {spread(1e3 * x for x in r['rounds_torch'])} |")
    L += ["", "Dispatch included on both sides (a burst of launches, one synchronise).  At 64 the kernel is the copy of the three channels.", "",
          "## `ffno_energy_spectrum` alone (200 calls per round; half spectra ready on the device)", "",
          "| images of 64 x 64 | kernel, us | torch ops, us | the batched `rfft2` in front of it, us | largest relative difference | rounds (kernel / torch) |",
          "|---|---|---|---|---|---|"]
    for r in rows["spectrum"]:
        L.append(f"| {r['images']} | **{r['kernel_us']:.2f}** | {r['torch_ops_us']:.2f} | {r['rfft2_us']:.2f} | {r['max_rel_diff']:.2e} | "
                 f"{spread(1e3 * x for x in r['rounds_kernel'])} / {spread(1e3 * x for x in r['rounds_torch'])} |")
    L += ["", "The torch side sums with `index_add_` (atomics: its bits change from run to run); the kernel's order is fixed.", "",
          "## The C-ABI calls of one test batch", "",
          "Per entry point, without / with the export; identical where one number stands.  `ffno_velocity_features` is three kernels, every",
          "other launching entry point one; `*_supported` and `*_ws_floats` are host-side queries.  One rollout step is a tenth of the",
          "per-step entries.", ""]
    names = sorted({n for r in rows["calls"] for n in (*r["with_export"], *r["without"])})
    L += ["| entry point | " + " | ".join(f"{r['grid']} x {r['grid']}" for r in rows["calls"]) + " |", "|---|" + "---|" * len(rows["calls"])]
    for n in names:
        cells = []
        for r in rows["calls"]:
            a, b = r["without"].get(n, 0), r["with_export"].get(n, 0)
            cells.append(str(a) if a == b else f"{a} / {b}")
        L.append(f"| `{n}` | " + " | ".join(cells) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(output)), exist_ok=True)
    with open(output, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "pred_export.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_pred_export.py measures on the GPU; none is visible")
    main(args.output)
