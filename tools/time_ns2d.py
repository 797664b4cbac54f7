"""Time per solver step of `generate navier-stokes` at the reference's defaults -- batch 50, grid 256 x 256, delta 1e-4, the `li`
force, viscosity 1e-5 -- against a torch-eager fp32 evaluation of the same step (the restatement of tests/ns2d_oracle.py: full
complex FFTs, tables computed once; it is leaner than the reference's own loop, which clones and assigns real / imaginary parts
separately), on the same GPU in the same process.  The two sides alternate (--rounds rounds of --steps steps each after a warm-up,
HIP events around each burst, median over the rounds), and the tool reports how far the two runs are apart afterwards.  Run from
the repository root; prints one JSON document.  --hip-only runs just the HIP side: the process to put under a kernel trace.

--varying-force times three kinds of step instead, alternating in the same way, with the random force (cycles 2, scaling 0.1,
t_scaling 0.2): (a) the time-varying force as built, ffno_ns2d_cn_update_harmonic from the amplitudes and the phase; (b) a constant
per-sample force, the update that streams f_h [B, N, N/2+1]; (c) the time-varying force as a plain port: the field from torch
sin / cos over [B, N, N] at the step's time (grids computed once, leaner than the reference, which rebuilds them every step), its
rfft2, then the update of (b)."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch  # noqa: E402

import ns2d_oracle as oracle  # noqa: E402
from fourierflow_amd.builders import GaussianRF  # noqa: E402
from fourierflow_amd.builders.synthetic import Force, SpectralStepper, _force_field, _unit_grid, random_force_amplitudes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--grid", type=int, default=256)
ap.add_argument("--hip-only", action="store_true")
ap.add_argument("--varying-force", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, N, DT, NU = a.batch, a.grid, 1e-4, 1e-5

torch.manual_seed(0)
w0 = GaussianRF(2, N, alpha=2.5, tau=7, device=dev).sample(B)
nu = torch.full((B,), NU, dtype=torch.float32, device=dev)


def burst(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def time_varying_force():
    cycles, scaling, t_scaling = 2, 0.1, 0.2
    amp = random_force_amplitudes(B, dev, cycles, 1)
    clock = dict(a=0.0, c=0.0)
    harmonic = SpectralStepper(w0, nu, None, DT, harmonic=(amp, scaling))
    constant = SpectralStepper(w0, nu, _force_field(Force.random, B, N, dev, cycles, scaling, 1), DT)
    port = SpectralStepper(w0, nu, torch.zeros(B, N, N, device=dev), DT)
    X, Y = (g.expand(B, N, N).contiguous() for g in _unit_grid(N, dev))

    def step_a():
        harmonic.step(t_scaling * clock["a"])
        clock["a"] += DT

    def step_c():
        ph, f = t_scaling * clock["c"], 0
        for p in range(1, cycles + 1):
            k = 2 * math.pi * p
            for i, (wave, arg) in enumerate(((torch.sin, X), (torch.cos, X), (torch.sin, Y), (torch.cos, Y), (torch.sin, X + Y),
                                             (torch.cos, X + Y))):
                f = f + amp[p - 1, i][:, None, None] * wave(k * arg + ph)
        port.f_h = torch.view_as_real(torch.fft.rfft2(f * scaling)).contiguous()
        port.step()
        clock["c"] += DT

    kinds = dict(harmonic=step_a, constant=constant.step, port=step_c)
    with torch.no_grad():
        for _ in range(10):
            for step in kinds.values():
                step()
        torch.cuda.synchronize()
        rounds = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for k, step in kinds.items():
                rounds[k].append(burst(step, a.steps))
        w_a, w_c = harmonic.vorticity(), port.vorticity()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    print(json.dumps(dict(shape=dict(B=B, N=N, delta=DT, visc=NU, force="random", cycles=cycles, scaling=scaling, t_scaling=t_scaling),
                          steps_per_burst=a.steps, rounds=a.rounds,
                          us_per_step={k: round(v, 1) for k, v in med.items()},
                          rounds_us={k: [round(t, 1) for t in v] for k, v in rounds.items()},
                          harmonic_over_constant=round(med["harmonic"] / med["constant"], 4),
                          port_over_harmonic=round(med["port"] / med["harmonic"], 3),
                          total_steps_each=10 + a.steps * a.rounds,
                          rel_l2_harmonic_vs_port=float("%.2e" % ((w_a - w_c).norm() / w_c.norm()).item())), indent=1))


if a.varying_force:
    time_varying_force()
    sys.exit(0)

f = _force_field(Force.li, B, N, dev, None, None, 0)
hip = SpectralStepper(w0, nu, f, DT)


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
