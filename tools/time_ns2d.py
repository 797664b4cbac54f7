"""Time per solver step of `generate navier-stokes` at the reference's defaults -- batch 50, grid 256 x 256, delta 1e-4, the `li`
force, viscosity 1e-5 -- against a torch-eager fp32 evaluation of the same step (the restatement of tests/ns2d_oracle.py: full
complex FFTs, tables computed once; it is leaner than the reference's own loop, which clones and assigns real / imaginary parts
separately), on the same GPU in the same process.  The two sides alternate (--rounds rounds of --steps steps each after a warm-up,
HIP events around each burst, median over the rounds), and the tool reports how far the two runs are apart afterwards.  Run from
the repository root; prints one JSON document.  --hip-only runs just the HIP side: the process to put under a kernel trace."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch  # noqa: E402

import ns2d_oracle as oracle  # noqa: E402
from fourierflow_amd.builders import GaussianRF  # noqa: E402
from fourierflow_amd.builders.synthetic import Force, SpectralStepper, _force_field  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--grid", type=int, default=256)
ap.add_argument("--hip-only", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, N, DT, NU = a.batch, a.grid, 1e-4, 1e-5

torch.manual_seed(0)
w0 = GaussianRF(2, N, alpha=2.5, tau=7, device=dev).sample(B)
nu = torch.full((B,), NU, dtype=torch.float32, device=dev)
f = _force_field(Force.li, B, N, dev, None, None, 0)
hip = SpectralStepper(w0, nu, f, DT)


def burst(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


if a.hip_only:
    for _ in range(a.steps):
        hip.step()
    torch.cuda.synchronize()
    print(json.dumps(dict(steps=a.steps, B=B, N=N, finite=bool(torch.isfinite(hip.vorticity()).all()))))
    sys.exit(0)

tabs = oracle.tables(N, torch.float32, dev)
state = dict(w_h=torch.fft.fft2(w0), f_h=torch.fft.fft2(f))


def eager_step():
    state["w_h"] = oracle.step(state["w_h"], state["f_h"], nu, DT, tabs)


with torch.no_grad():
    for _ in range(10):
        hip.step()
        eager_step()
    torch.cuda.synchronize()
    t_hip, t_eager = [], []
    for _ in range(a.rounds):
        t_hip.append(burst(hip.step, a.steps))
        t_eager.append(burst(eager_step, a.steps))
    w_hip, w_eager = hip.vorticity(), torch.fft.ifft2(state["w_h"]).real
h, e = statistics.median(t_hip), statistics.median(t_eager)
print(json.dumps(dict(shape=dict(B=B, N=N, delta=DT, visc=NU, force="li"), steps_per_burst=a.steps, rounds=a.rounds,
                      hip_us_per_step=round(h, 1), eager_us_per_step=round(e, 1), eager_over_hip=round(e / h, 2),
                      hip_rounds_us=[round(t, 1) for t in t_hip], eager_rounds_us=[round(t, 1) for t in t_eager],
                      total_steps_each=10 + a.steps * a.rounds,
                      rel_l2_hip_vs_eager=float("%.2e" % ((w_hip - w_eager).norm() / w_eager.norm()).item())), indent=1))
