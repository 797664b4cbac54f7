#!/usr/bin/env python3
"""What the reduced-grid correlation costs in the validation of a torus_kochkov routine (24 layers, width 64, 16 modes,
use_velocity, batch 32, 10 steps) on the GPU.  profiles/kolmogorov_builder.md holds the output.

  valid     ms per validation batch with corr_data at the model's own size (no reduction: the path before downsample_corr)
            against corr_data at 32 x 32 through ffno_velocity_features + ffno_vorticity_coarsen_step, at 64 x 64 and 128 x 128;
            median of 5 rounds of 10 calls, the two sides alternating
  coarsen   ffno_vorticity_coarsen_step alone against the same arithmetic written with torch ops on the device (strided
            slices, two means, two rolls, three sums), 64 -> 32 and 128 -> 32; median of 5 rounds of 200 calls, alternating;
            the largest difference between the two results goes along
  calls     the C-ABI calls of one validation batch, by entry point (ffno_velocity_features is three kernels, every other
            entry point counted here one)
  p2_error  max |p_2 - float64| of tests/test_markov_reduced_corr.py's two cases on this device

One JSON line each.  Run from the repository root:  python tools/time_reduced_corr.py"""
import collections
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fourierflow_amd import _capi, _lib  # noqa: E402
from fourierflow_amd._lib import ptr as _p  # noqa: E402
from fourierflow_amd.modules import FNOFactorized2DBlock  # noqa: E402
from fourierflow_amd.routines import Grid2DMarkovExperiment  # noqa: E402

KW = dict(modes=16, width=64, n_layers=24, input_dim=5, share_weight=False, factor=4, ff_weight_norm=True, gain=0.1)
B, T, N, M2 = 32, 11, 10, 32
dev = "cuda:0"
TWO_PI = 2 * math.pi


def sync_time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps, r


def alternate(a, b, reps, rounds=5):
    for fn in (a, b):
        sync_time(fn, 3)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(sync_time(a, reps)[0])
        tb.append(sync_time(b, reps)[0])
    return statistics.median(ta), statistics.median(tb), ta, tb


def routine(G):
    torch.manual_seed(0)
    exp = Grid2DMarkovExperiment(FNOFactorized2DBlock(**KW), use_velocity=True, grid_size=[G], step_size=0.28,
                                 downsample_corr=True).to(dev)
    for _ in range(2):
        exp.training_step(dict(x=torch.randn(B, G, G, 1, device=dev), y=torch.randn(B, G, G, 1, device=dev)), epoch=0)
    return exp.eval()


def count_calls(fn):
    """{entry point: calls} of one fn(): every bound function of the library object is wrapped for the duration."""
    lib, counts, saved = _lib.get_lib(), collections.Counter(), {}
    for name in _capi.SIGNATURES:
        saved[name] = getattr(lib, name)

        def wrapped(*a, _f=saved[name], _n=name):
            counts[_n] += 1
            return _f(*a)
        setattr(lib, name, wrapped)
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    return dict(sorted(counts.items()))


def torch_coarsen(vel, corr_t, m, lx, ly):
    """The arithmetic of ffno_vorticity_coarsen_step on the device with torch ops -> (w_c, the three per-sample sums)."""
    Bv, X, Y, _ = vel.shape
    f = X // m
    u_c = vel[:, f - 1::f, :, 1].reshape(Bv, m, m, f).mean(-1)
    v_c = vel[:, :, f - 1::f, 2].reshape(Bv, m, f, m).mean(2)
    w = (torch.roll(v_c, -1, 1) - v_c) / (lx / m) - (torch.roll(u_c, -1, 2) - u_c) / (ly / m)
    return w, torch.stack([(w * w).sum((1, 2)), (corr_t * corr_t).sum((1, 2)), (w * corr_t).sum((1, 2))], -1)


def main():
    lib = _lib.get_lib()
    for G in (64, 128):
        exp = routine(G)
        data = torch.randn(B, G, G, T, device=dev)
        own = dict(data=data, corr_data=torch.randn(B, G, G, T, device=dev))
        red = dict(data=data, corr_data=torch.randn(B, M2, M2, T, device=dev))
        t_own, t_red, r_own, r_red = alternate(lambda: exp.validation_step(own), lambda: exp.validation_step(red), 10)
        print(json.dumps(dict(what="valid", grid=G, corr=M2, batch=B, n_steps=N, own_size_ms=t_own, reduced_ms=t_red,
                              rounds_own=r_own, rounds_reduced=r_red)), flush=True)
        print(json.dumps(dict(what="calls", grid=G, own_size=count_calls(lambda: exp.validation_step(own)),
                              reduced=count_calls(lambda: exp.validation_step(red)))), flush=True)
        # the launch alone
        vel = torch.randn(B, G, G, 3, device=dev)
        corr = red["corr_data"]
        sums = torch.empty(int(lib.ffno_vorticity_coarsen_ws_floats(B, M2, N)), device=dev)
        preds2 = torch.empty(B, M2, M2, N, device=dev)
        stream = _lib.current_stream(vel.device)

        def kernel():
            _capi.check(lib.ffno_vorticity_coarsen_step(_p(vel), _p(corr), _p(preds2), _p(sums), B, G, G, M2, T, N, 0, TWO_PI, TWO_PI,
                                                        stream), "vorticity_coarsen_step")

        def eager():
            return torch_coarsen(vel, corr[..., T - N], M2, TWO_PI, TWO_PI)

        t_k, t_e, r_k, r_e = alternate(kernel, eager, 200)
        w, s = eager()
        S = sums.numel() // (N * B * 3)
        diff_w = float((preds2[..., 0] - w).abs().max())
        diff_s = float(((sums.view(N, B, S, 3)[0].sum(1) - s).abs() / s.abs().clamp_min(1e-30)).max())
        print(json.dumps(dict(what="coarsen", grid=G, corr=M2, batch=B, kernel_ms=t_k, torch_ops_ms=t_e, rounds_kernel=r_k,
                              rounds_torch=r_e, max_abs_diff_w=diff_w, max_rel_diff_sums=diff_s)), flush=True)
        del exp
    # the deviation of p_2 from float64 that tests/test_markov_reduced_corr.py bounds, on this device
    import coarsen_oracle as co
    import test_markov_reduced_corr as tm
    for use_velocity in (False, True):
        exp = tm._routine(dev, use_velocity, downsample_corr=True)
        batch = tm._data(dev)
        preds = tm._own_preds(exp, batch)
        wc = co.downsample_vorticity(preds, tm.M2, tm.LX, tm.LY)
        corr = tm._noisy_corr(wc, (0.05, 0.2, 0.6, 2.0), 3)
        batch["corr_data"] = torch.from_numpy(corr).to(dev)
        want, _ = co.correlation(wc, corr, tm.N_STEPS)
        loss_sum, _, again, _ = exp._valid_step(batch)
        p = exp.compute_losses(batch, loss_sum, again)[4].cpu().numpy().astype(np.float64)
        print(json.dumps(dict(what="p2_error", use_velocity=use_velocity, max_abs=float(np.abs(p - want).max()))), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("time_reduced_corr.py measures on the GPU; none is visible")
    main()
