"""solve_navier_stokes_2d and GaussianRF against recordings of the reference's own ns_2d.py / random_fields.py
(tests/golden/ns2d_ref.npz, written by tools/make_golden_ns2d.py on the CPU in fp32): N = 16, B = 3, 10 steps, two snapshots,
the forces li / kolmogorov / none / random, each with a scalar and a per-sample viscosity.  Bound: 1e-5 relative L2 per snapshot.

The reference draws the seed of its random force from numpy and the amplitudes from a torch generator on the solver's device.
On CPU tensors the solver here, numpy seeded alike, reproduces the recorded force.  A generator on the GPU draws other numbers,
so there the recorded force field is handed to the solver in place of its own draw."""
import os

import numpy as np
import pytest
import torch

import ns2d_oracle as oracle
from backend_util import host_device  # noqa: F401
from fourierflow_amd.builders import Force, GaussianRF, solve_navier_stokes_2d, synthetic

G = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ns2d_ref.npz")))
B, N, STEPS, RECORDS, CYCLES, NUMPY_SEED, GRF_SEED = (int(v) for v in G["shape"])
DT, SCALING = float(G["dt"]), float(G["scaling"])


def test_gaussian_rf_is_the_reference_on_the_same_seed():
    torch.manual_seed(GRF_SEED)       # (the CPU generator: the recording's)
    u = GaussianRF(2, N, alpha=2.5, tau=7, device="cpu").sample(B)
    assert oracle.rel_l2(u.numpy(), G["grf"]) <= 1e-6


@pytest.mark.parametrize("visc", ["scalar", "array"])
@pytest.mark.parametrize("force", ["li", "kolmogorov", "none", "random"])
def test_solver_reproduces_the_reference(host_device, monkeypatch, force, visc):
    if force == "random" and host_device != "cpu":
        recorded = torch.from_numpy(G["random.f"]).to(host_device)
        monkeypatch.setattr(synthetic, "random_force", lambda *a, **k: recorded)
    nu = float(G["visc_scalar"]) if visc == "scalar" else G["visc_array"]
    np.random.seed(NUMPY_SEED)
    sol, f = solve_navier_stokes_2d(torch.from_numpy(G["w0"]).to(host_device), nu, STEPS * DT, DT, RECORDS, CYCLES, SCALING, 0.2,
                                    Force(force), False)
    if force == "none":
        assert f is None
    else:
        # (two fp32 evaluations of sin / cos whose fp32 arguments, up to 8 pi, may differ by an ulp: 2e-6)
        assert f.shape == G[f"{force}.f"].shape and oracle.rel_l2(f, G[f"{force}.f"]) <= 2e-6
    ref = G[f"{force}.{visc}.sol"]
    assert oracle.rel_l2(ref[..., -1], G["w0"]) > 1e-2      # the recorded flow moves
    errs = [oracle.rel_l2(sol[..., i], ref[..., i]) for i in range(RECORDS)]
    print(f"[ns2d golden {force} visc={visc}] " + " ".join(f"{e:.2e}" for e in errs))
    assert sol.shape == ref.shape and max(errs) <= 1e-5, errs
