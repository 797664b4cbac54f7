"""solve_navier_stokes_2d_varying_force -- the reference's solve_navier_stokes_2d(..., varying_force=True), an entry of its own
here because solve_navier_stokes_2d keeps its refusal of that argument -- against recordings of the reference's own ns_2d.py
(tests/golden/ns2d_varying_ref.npz, written by tools/make_golden_ns2d_varying.py on the CPU in fp32): the initial vorticity,
viscosities, grid (N = 16, B = 3), steps (10 of 1e-2, two snapshots) and numpy seed of tests/golden/ns2d_ref.npz, the random force
with t_scaling = 20 and 0.2.  Bounds, those of test_ns2d_golden.py for the same solver, grid and step count: 1e-5 relative L2 for
every snapshot, 2e-6 for every recorded force.  At t_scaling = 20 a force frozen at t = 0 is 2.8e-3 off in the solution, one a
step late 1.4e-3, and a force recorded at the snapshot's time 0.2 off in the force; at 0.2 a one-step slip is 1.1e-5.

The reference draws the seed of its force from numpy and the amplitudes from a torch generator on the solver's device.  On CPU
tensors the solver here, numpy seeded alike, draws the recorded amplitudes itself.  A generator on the GPU draws other numbers,
so there the recorded amplitudes are handed to the solver in place of its own draw."""
import os

import numpy as np
import pytest
import torch

import ns2d_oracle as oracle
from backend_util import host_device  # noqa: F401
from fourierflow_amd.builders import Force, solve_navier_stokes_2d_varying_force, synthetic

G = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ns2d_varying_ref.npz")))
B, N, STEPS, RECORDS, CYCLES, NUMPY_SEED, _ = (int(v) for v in G["shape"])
DT, SCALING = float(G["dt"]), float(G["scaling"])


def _solve(host_device, monkeypatch, force, visc, t_scaling):
    if host_device != "cpu":
        recorded = torch.from_numpy(G["amplitudes"]).to(host_device)
        monkeypatch.setattr(synthetic, "random_force_amplitudes", lambda *a, **k: recorded)
    nu = float(G["visc_scalar"]) if visc == "scalar" else G["visc_array"]
    np.random.seed(NUMPY_SEED)
    return solve_navier_stokes_2d_varying_force(torch.from_numpy(G["w0"]).to(host_device), nu, STEPS * DT, DT, RECORDS, CYCLES, SCALING,
                                                t_scaling, Force(force))


def _compare(tag, sol, fs, ref_sol, ref_fs):
    assert isinstance(sol, np.ndarray) and isinstance(fs, np.ndarray) and sol.dtype == fs.dtype == np.float32
    assert sol.shape == ref_sol.shape == (B, N, N, RECORDS) and fs.shape == ref_fs.shape == (B, N, N, RECORDS)
    errs = [oracle.rel_l2(sol[..., i], ref_sol[..., i]) for i in range(RECORDS)]
    ferrs = [oracle.rel_l2(fs[..., i], ref_fs[..., i]) for i in range(RECORDS)]
    print(f"[ns2d varying golden {tag}] sol " + " ".join(f"{e:.2e}" for e in errs) + "  fs " + " ".join(f"{e:.2e}" for e in ferrs))
    assert max(errs) <= 1e-5, errs
    assert max(ferrs) <= 2e-6, ferrs


def test_the_seeded_draw_gives_the_recorded_amplitudes():
    np.random.seed(NUMPY_SEED)
    a = synthetic.random_force_amplitudes(B, "cpu", CYCLES, int(np.random.randint(1, 1000000000)))
    assert a.shape == (CYCLES, 6, B) and a.dtype == torch.float32
    np.testing.assert_array_equal(a.numpy(), G["amplitudes"])


@pytest.mark.parametrize("visc", ["scalar", "array"])
@pytest.mark.parametrize("t_scaling", [20.0, 0.2])
def test_solver_reproduces_the_reference(host_device, monkeypatch, t_scaling, visc):
    ref_sol, ref_fs = G[f"random.{t_scaling:g}.{visc}.sol"], G[f"random.{t_scaling:g}.fs"]
    assert oracle.rel_l2(ref_sol[..., -1], G["w0"]) > 1e-2      # the recorded flow moves
    if t_scaling == 20.0:      # ... and the recorded force varies (at 0.2 the phase moves 0.01 rad between the two snapshots)
        assert oracle.rel_l2(ref_fs[..., 0], ref_fs[..., 1]) > 1e-2
    sol, fs = _solve(host_device, monkeypatch, "random", visc, t_scaling)
    _compare(f"t_scaling={t_scaling:g} visc={visc}", sol, fs, ref_sol, ref_fs)


def test_li_with_varying_force_is_the_random_force(host_device, monkeypatch):
    """The reference calls the random force whatever the force is, once varying_force is set."""
    np.testing.assert_array_equal(G["li.20.fs"], G["random.20.fs"])
    sol, fs = _solve(host_device, monkeypatch, "li", "scalar", 20.0)
    _compare("li", sol, fs, G["li.20.scalar.sol"], G["li.20.fs"])


def test_refusals(host_device):
    w0 = torch.from_numpy(G["w0"]).to(host_device)
    with pytest.raises(ValueError, match="Force.none"):
        solve_navier_stokes_2d_varying_force(w0, 1e-3, STEPS * DT, DT, RECORDS, CYCLES, SCALING, 20.0, Force.none)
    for missing in ((None, SCALING, 20.0), (CYCLES, None, 20.0), (CYCLES, SCALING, None)):
        with pytest.raises(ValueError, match="cycles, scaling and t_scaling"):
            solve_navier_stokes_2d_varying_force(w0, 1e-3, STEPS * DT, DT, RECORDS, *missing, Force.random)
    with pytest.raises(ValueError, match="cycles"):      # p = N/2: the rows p and N - p of the half spectrum coincide
        solve_navier_stokes_2d_varying_force(w0, 1e-3, STEPS * DT, DT, RECORDS, N // 2, SCALING, 20.0, Force.random)
