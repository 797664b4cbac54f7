"""Times of the fully factorised point-cloud F-FNO (FNOFullyFactorizedMesh2D + IPhi under PointCloudExperiment, AdamW) on the GPU,
beside FNOFactorizedPointCloud2D at the same shape in the same process.  Writes profiles/pointcloud_fullyfact.md (``--out``).

1. At batch 20 x 972 points, 4 layers and (width, modes, grid) = (32, 12, 40) and (64, 16, 64): ms per forward (no_grad) and per
   training step of both models, alternating bursts, the median over the rounds and the spread (max - min over the rounds); and
   the library launches of one training step (torch's own glue kernels -- cat, einsum, permute copies -- are not counted).
2. us of each new launch alone at both shapes (ffno_nudft_axis_modes on the 3 channels of layer 0 and on W channels as the
   adjoint, ffno_nudft_axis_points forward / with dxi, ffno_axis_modes_to_grid, ffno_grid_to_axis_modes), and ffno_nudft_modes /
   ffno_nudft_points at the same (m1, m2) and channel counts, alternating with them.  The 2-D kernels take at most 16 modes.

Device-event pairs around bursts of back-to-back calls; every shape is warmed up first.  Run from the repository root."""
import argparse
import collections
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from fourierflow_amd import _capi, _lib  # noqa: E402
from fourierflow_amd.modules import FNOFactorizedPointCloud2D, FNOFullyFactorizedMesh2D, IPhi  # noqa: E402
from fourierflow_amd.routines import PointCloudExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200, help="calls per burst of a single launch")
ap.add_argument("--step-iters", type=int, default=50, help="forwards / training steps per burst")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--out", default=os.path.join("profiles", "pointcloud_fullyfact.md"))
ap.add_argument("--rehearse", action="store_true",
                help="tiny shapes through the CPU emulator build of the tests: checks the tool's plumbing, its times mean nothing")
a = ap.parse_args()
if a.rehearse:
    os.environ.setdefault("FFNO_ALLOW_TEST_BACKEND", "1")
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import backend_util
    _lib._install_test_backend(backend_util.emu_lib())
elif not torch.cuda.is_available():
    sys.exit("time_pointcloud_fullyfact.py measures on the GPU and found none (use --rehearse to check the plumbing)")
dev = torch.device("cpu" if a.rehearse else "cuda:0")
lib = _lib.get_lib()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sync():
    if not a.rehearse:
        torch.cuda.synchronize()


def burst(f, n):
    """time of one call of f in a burst of n, in us"""
    if a.rehearse:
        import time
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        return (time.perf_counter() - t0) * 1e6 / n
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def alternate(fs, n):
    """{name: (median, spread)} over a.rounds rounds, one burst of every f per round"""
    for f in fs.values():
        for _ in range(3):
            f()
    sync()
    t = {k: [] for k in fs}
    for _ in range(a.rounds):
        for k, f in fs.items():
            t[k].append(burst(f, n))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}


def launches(f):
    counts = collections.Counter()
    real = _capi.check

    def counting(rc, what):
        counts[what] += 1
        return real(rc, what)
    _capi.check = counting
    try:
        f()
    finally:
        _capi.check = real
    sync()
    return counts


B, N, L = (2, 37, 2) if a.rehearse else (20, 972, 4)
SHAPES = [(32, 3, 8, 16)] if a.rehearse else [(32, 12, 40, 32), (64, 16, 64, 64)]      # (width, modes, grid, IPhi width)
lines = ["# The fully factorised point-cloud F-FNO on an MI355X", "",
         f"`python tools/time_pointcloud_fullyfact.py` (device-event pairs around bursts of back-to-back calls, {a.rounds} rounds, the two",
         "sides of every comparison alternating in one process; median, and spread = max - min over the rounds).",
         f"Batch {B} x {N} points, {L} layers, AdamW; `FNOFullyFactorizedMesh2D` beside `FNOFactorizedPointCloud2D` at the same shape.", ""]
if a.rehearse:
    lines.insert(1, "\n**Rehearsal on the CPU emulator: the times below mean nothing.**")

g = torch.Generator().manual_seed(0)
batch = dict(xy=torch.rand(B, N, 2, generator=g).to(dev), rr=torch.randn(B, 42, generator=g).to(dev),
             sigma=torch.randn(B, N, 1, generator=g).to(dev))
lines += ["## Model: ms per forward and per training step", "",
          "| width, modes, grid | model | forward ms (spread) | training step ms (spread) | library launches per step |", "|---|---|---|---|---|"]
by_entry = {}
for W, M, S, IW in SHAPES:
    torch.manual_seed(2)
    routines = {
        "FNOFullyFactorizedMesh2D": PointCloudExperiment(FNOFullyFactorizedMesh2D(M, M, W, 2, 1, n_layers=L, s1=S, s2=S).to(dev),
                                                         IPhi(IW).to(dev), 1000),
        "FNOFactorizedPointCloud2D": PointCloudExperiment(FNOFactorizedPointCloud2D(M, M, W, 2, 1, n_layers=L, s1=S, s2=S).to(dev),
                                                          IPhi(IW).to(dev), 1000),
    }

    def forward(r):
        with torch.no_grad():
            return r(batch)
    fwd = alternate({k: (lambda r=r: forward(r)) for k, r in routines.items()}, a.step_iters)
    step = alternate({k: (lambda r=r: r.training_step(batch)) for k, r in routines.items()}, a.step_iters)
    for k, r in routines.items():
        counts = launches(lambda r=r: r.training_step(batch))
        by_entry[(W, M, S, k)] = counts
        lines.append(f"| {W}, {M}, {S} | `{k}` | {fwd[k][0] / 1000:.3f} ({fwd[k][1] / 1000:.3f}) | {step[k][0] / 1000:.3f} "
                     f"({step[k][1] / 1000:.3f}) | {sum(counts.values())} |")
lines += ["", "Library launches of one training step by entry point (the label each call is checked under):", ""]
for (W, M, S, k), counts in by_entry.items():
    lines.append(f"- width {W}, `{k}`: " + ", ".join(f"{n} x {c}" for n, c in sorted(counts.items())))

lines += ["", "## Launches alone: us per call", "",
          "| width, modes, grid | launch | per-axis us (spread) | 2-D counterpart | 2-D us (spread) |", "|---|---|---|---|---|"]
st = _lib.current_stream(dev)
for W, M, S, _ in SHAPES:
    K = 2 * M
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
    e = lambda *shape: torch.empty(*shape, device=dev)                 # noqa: E731
    xi = torch.rand(B, N, 2, generator=g).to(dev)
    u3, uW = rnd(B, 3, N), rnd(B, W, N)
    a3, aW, o3, oW, dxi = e(B, 3, K, 2), rnd(B, W, K, 2), e(B, 3, N), e(B, W, N), e(B, N, 2)
    aWo, a3s = e(B, W, K, 2), aW[:, :3].contiguous()
    s3, sW, sWo = e(B, 3, 2 * M, M, 2), rnd(B, W, 2 * M, M, 2), e(B, W, 2 * M, M, 2)
    grid, go = rnd(B, S, S, W), e(B, S, S, W)
    two_d = bool(lib.ffno_nudft_supported(W, M, M))
    ck = _capi.check
    pairs = [
        ("axis_modes, 3 channels (layer 0)", lambda: ck(lib.ffno_nudft_axis_modes(p(u3), p(xi), p(a3), B, 3, N, M, M, st), "m3"),
         "nudft_modes, 3 channels", lambda: ck(lib.ffno_nudft_modes(p(u3), p(xi), p(s3), B, 3, N, M, M, 0, st), "n3")),
        (f"axis_modes, {W} channels (adjoint of the last layer)",
         lambda: ck(lib.ffno_nudft_axis_modes(p(uW), p(xi), p(aWo), B, W, N, M, M, st), "mW"),
         f"nudft_modes, {W} channels", lambda: ck(lib.ffno_nudft_modes(p(uW), p(xi), p(sWo), B, W, N, M, M, 1, st), "nW")),
        (f"axis_points, {W} channels (last layer)",
         lambda: ck(lib.ffno_nudft_axis_points(p(aW), p(xi), None, p(oW), None, B, W, N, M, M, 0, st), "pW"),
         f"nudft_points, {W} channels", lambda: ck(lib.ffno_nudft_points(p(sW), p(xi), None, p(oW), None, B, W, N, M, M, 1, 0, st), "qW")),
        (f"axis_points, {W} channels, dxi only",
         lambda: ck(lib.ffno_nudft_axis_points(p(aW), p(xi), p(uW), None, p(dxi), B, W, N, M, M, 0, st), "pd"),
         f"nudft_points, {W} channels, dxi only",
         lambda: ck(lib.ffno_nudft_points(p(sW), p(xi), p(uW), None, p(dxi), B, W, N, M, M, 1, 0, st), "qd")),
        ("axis_points, 3 channels, out + dxi (adjoint of layer 0)",
         lambda: ck(lib.ffno_nudft_axis_points(p(a3s), p(xi), p(u3), p(o3), p(dxi), B, 3, N, M, M, 0, st), "p3"),
         None, None),
        ("axis_modes_to_grid (c2r)", lambda: ck(lib.ffno_axis_modes_to_grid(p(aW), p(go), B, W, S, M, M, 1, st), "tg"), None, None),
        ("grid_to_axis_modes (plain)", lambda: ck(lib.ffno_grid_to_axis_modes(p(grid), p(aWo), B, W, S, M, M, 0, st), "tm"), None, None),
    ]
    for name, f, name2, f2 in pairs:
        fs = {"axis": f}
        if f2 is not None and two_d:
            fs["two_d"] = f2
        t = alternate(fs, a.iters)
        other = f"{name2} | {t['two_d'][0]:.1f} ({t['two_d'][1]:.1f})" if "two_d" in t else "- | -"
        lines.append(f"| {W}, {M}, {S} | {name} | {t['axis'][0]:.1f} ({t['axis'][1]:.1f}) | {other} |")

os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
