"""Time per time step of `generate kolmogorov` (five RK stages: KolmogorovStepper.step) at 256 x 256 x 8 and 2048 x 2048 x 1 with
the shipped re_1000 physics -- viscosity 1e-3, drag 0.1, forcing wavenumber 4, the time step of stable_time_step -- against a
torch-eager fp32 evaluation of the same formulas (the restatement of tests/kf2d_oracle.py in torch: full complex FFTs, tables
computed once), on the same GPU in the same process.  The two sides alternate (--rounds rounds of --steps steps each after a
warm-up, HIP events around each burst, median over the rounds).  The tool reports how far the two runs are apart after the
warm-up (three steps each) and at the end: the flow is chaotic, so over thousands of steps fp32 rounding grows to order one.
Run from the repository root; prints one JSON line per shape.  --hip-only runs just the HIP side of ONE shape (--grid, --batch):
the process to put under a kernel trace."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from fourierflow_amd.builders import KolmogorovStepper, initial_vorticity, stable_time_step  # noqa: E402
from fourierflow_amd.builders.kolmogorov_flow import ALPHA, BETA, GAMMA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=0, help="steps per burst; default 1000 up to 256 x 256, 200 above: a burst of the "
                                                     "HIP side is then about 0.3 s")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--grid", type=int, default=0, help="with --batch: this one shape instead of the two")
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--hip-only", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")
NU, DRAG, KF, MAG, MAX_V = 1e-3, 0.1, 4, 1.0, 7.0
SHAPES = [(a.grid, a.batch)] if a.grid and a.batch else [(256, 8), (2048, 1)]


class Eager:
    """The step in torch ops on full complex spectra, fp32."""

    def __init__(self, w0, dt):
        N = w0.shape[-1]
        i = torch.arange(N, device=dev)
        k = torch.where(i < N // 2, i, i - N).float()
        self.kx, self.ky = k[:, None].expand(N, N), k[None, :].expand(N, N)
        k2 = self.kx ** 2 + self.ky ** 2
        self.inv = torch.where(k2 > 0, 1.0 / k2.clamp_min(1.0), torch.zeros_like(k2))
        self.filt = (9 * k2 <= N * N).float()
        self.L = -NU * k2 - DRAG
        y = (torch.arange(N, device=dev).float() + 0.5) * (2 * math.pi / N)
        self.f_h = torch.fft.fft2((-MAG * KF * torch.cos(KF * y))[None, :].expand(N, N))
        self.w_h, self.dt = torch.fft.fft2(w0), dt

    def explicit(self, w_h):
        psi = w_h * self.inv
        vx, vy = torch.fft.ifft2(1j * self.ky * psi).real, torch.fft.ifft2(-1j * self.kx * psi).real
        w_x, w_y = torch.fft.ifft2(1j * self.kx * w_h).real, torch.fft.ifft2(1j * self.ky * w_h).real
        return -self.filt * torch.fft.fft2(vx * w_x + vy * w_y) + self.f_h

    def step(self):
        w_h, h = self.w_h, 0.0
        for s in range(5):
            h = self.explicit(w_h) + BETA[s] * h
            mu = 0.5 * self.dt * (ALPHA[s + 1] - ALPHA[s])
            w_h = (w_h + GAMMA[s] * self.dt * h + mu * self.L * w_h) / (1 - mu * self.L)
        self.w_h = w_h


def burst(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


for N, B in SHAPES:
    dt = stable_time_step(MAX_V, 0.5, NU, 2 * math.pi / N)
    steps = a.steps or (1000 if N <= 256 else 200)
    w0 = initial_vorticity(B, N, MAX_V, 4.0, 0, device=dev)
    hip = KolmogorovStepper(w0, NU, DRAG, dt, KF, MAG)
    if a.hip_only:
        for _ in range(steps):
            hip.step()
        torch.cuda.synchronize()
        print(json.dumps(dict(steps=steps, B=B, N=N, finite=bool(torch.isfinite(hip.vorticity()).all()))), flush=True)
        continue
    eager = Eager(w0, dt)
    with torch.no_grad():
        for _ in range(3):
            hip.step()
            eager.step()
        torch.cuda.synchronize()

        def apart():
            w_hip, w_eager = hip.vorticity(), torch.fft.ifft2(eager.w_h).real
            return float("%.2e" % ((w_hip - w_eager).norm() / w_eager.norm()).item())

        after_warmup = apart()
        t_hip, t_eager = [], []
        for _ in range(a.rounds):
            t_hip.append(burst(hip.step, steps))
            t_eager.append(burst(eager.step, steps))
    h, e = statistics.median(t_hip), statistics.median(t_eager)
    print(json.dumps(dict(shape=dict(B=B, N=N, dt=dt, viscosity=NU, drag=DRAG, forcing_wavenumber=KF), steps_per_burst=steps,
                          rounds=a.rounds, hip_us_per_step=round(h, 1), eager_us_per_step=round(e, 1), eager_over_hip=round(e / h, 2),
                          hip_rounds_us=[round(t, 1) for t in t_hip], eager_rounds_us=[round(t, 1) for t in t_eager],
                          total_steps_each=3 + steps * a.rounds, rel_l2_hip_vs_eager_after_warmup=after_warmup,
                          rel_l2_hip_vs_eager_at_end=apart(), finite=bool(torch.isfinite(hip.vorticity()).all()))), flush=True)
