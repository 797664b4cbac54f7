"""solve_navier_stokes_2d_varying_force (the reference's solve_navier_stokes_2d(..., varying_force=True)) against a float64
loop: tests/ns2d_oracle.py's step in its full complex FFT form, fed at every step with fft2 of the force evaluated plainly on the
grid at that step's time.  N = 16, B = 3, 10 steps of 1e-2
at t_scaling = 20 (0.2 rad a step) from a white-noise vorticity; the amplitudes are handed to the solver on both backends.
Bound: 1e-5 relative L2 per snapshot (test_ns2d_solver.py's, same grid and step count); the recorded forces, 2e-6 (as there)."""
import math

import numpy as np
import pytest
import torch

import ns2d_oracle as oracle
from backend_util import host_device  # noqa: F401
from fourierflow_amd.builders import Force, solve_navier_stokes_2d_varying_force, synthetic

B, N, STEPS, DT = 3, 16, 10, 1e-2
CYCLES, SCALING, T_SCALING = 2, 0.1, 20.0
VISC = {"scalar": 1e-3, "array": np.array([1e-3, 2e-3, 5e-4])}
AMP = np.random.default_rng(8).random((CYCLES, 6, B)).astype(np.float32)
W0 = np.random.default_rng(5).standard_normal((B, N, N)).astype(np.float32)
_REF = {}


def _force(t):
    """[B, N, N] float64: scaling sum_p a sin / cos (2 pi p {x, y, x + y} + t_scaling t)."""
    g = torch.arange(N, dtype=torch.float64) / N
    X, Y = g[:, None].expand(N, N), g[None, :].expand(N, N)
    a = torch.as_tensor(AMP, dtype=torch.float64)
    f = torch.zeros(B, N, N, dtype=torch.float64)
    for p in range(1, CYCLES + 1):
        k, ph = 2 * math.pi * p, T_SCALING * t
        terms = (torch.sin(k * X + ph), torch.cos(k * X + ph), torch.sin(k * Y + ph), torch.cos(k * Y + ph),
                 torch.sin(k * (X + Y) + ph), torch.cos(k * (X + Y) + ph))
        for i, term in enumerate(terms):
            f = f + a[p - 1, i][:, None, None] * term
    return SCALING * f


def _reference(visc, records):
    """(snapshots [B, N, N, records], the force of the last step before each, the force at each snapshot's time), float64."""
    if (visc, records) not in _REF:
        nu = torch.as_tensor(np.broadcast_to(np.asarray(VISC[visc], np.float64), (B,)).copy())
        tabs = oracle.tables(N, torch.float64)
        w_h = torch.fft.fft2(torch.as_tensor(W0, dtype=torch.float64))
        every, t = STEPS // records, 0.0
        sol, used, at_snapshot = [], [], []
        for j in range(every * records):
            f = _force(t)
            w_h = oracle.step(w_h, torch.fft.fft2(f), nu, DT, tabs)
            t += DT
            if (j + 1) % every == 0:
                sol.append(torch.fft.ifft2(w_h).real)
                used.append(f)
                at_snapshot.append(_force(t))
        _REF[visc, records] = tuple(torch.stack(x, dim=-1).numpy() for x in (sol, used, at_snapshot))
    return _REF[visc, records]


@pytest.mark.parametrize("visc", ["scalar", "array"])
@pytest.mark.parametrize("records", [5, 3])
def test_solver_follows_the_float64_loop(host_device, monkeypatch, records, visc):
    """records = 3: record_time = floor(10 / 3) = 3, snapshots after steps 3, 6, 9."""
    r64, f_used, f_at = _reference(visc, records)
    assert oracle.rel_l2(r64[..., -1], W0) > 1e-2                                  # the flow moves
    assert min(oracle.rel_l2(f_at[..., i], f_used[..., i]) for i in range(records)) > 0.1      # and a step of the force shows
    monkeypatch.setattr(synthetic, "random_force_amplitudes", lambda b, device, cycles, seed: torch.from_numpy(AMP).to(device))
    sol, fs = solve_navier_stokes_2d_varying_force(torch.from_numpy(W0).to(host_device), VISC[visc], STEPS * DT, DT, records, CYCLES,
                                                   SCALING, T_SCALING, Force.random)
    assert sol.shape == fs.shape == (B, N, N, records) and sol.dtype == fs.dtype == np.float32
    errs = [oracle.rel_l2(sol[..., i], r64[..., i]) for i in range(records)]
    ferrs = [oracle.rel_l2(fs[..., i], f_used[..., i]) for i in range(records)]
    print(f"[ns2d varying visc={visc} records={records}] sol " + " ".join(f"{e:.2e}" for e in errs) + "  fs " + " ".join(f"{e:.2e}" for e in ferrs))
    assert max(errs) <= 1e-5, errs
    assert max(ferrs) <= 2e-6, ferrs      # the force of the last step before each snapshot, not the one at its time
