"""solve_navier_stokes_2d and GaussianRF (fourierflow_amd/builders/synthetic.py) against the float64 restatement of
tests/ns2d_oracle.py, which runs the step in its full complex FFT form.  N = 16, B = 3, 10 steps of 1e-2 at viscosity 1e-3 from a
white-noise vorticity, so the Nyquist bins -- where the half-spectrum kernels have to write zeros to agree with that form -- carry
energy.  Every recorded snapshot is held to  max(1e-5, 4 x the float32 oracle's own distance from the float64 one)  (the band of
tests/test_pointcloud_model.py; that distance is about 3e-7 here, the solver's about 4e-7), on the emulator and on an MI355X."""
import numpy as np
import pytest
import torch

import ns2d_oracle as oracle
from backend_util import host_device  # noqa: F401
from fourierflow_amd.builders import Force, GaussianRF, solve_navier_stokes_2d

B, N, STEPS, DT, RECORDS = 3, 16, 10, 1e-2, 5
VISC = {"scalar": 1e-3, "array": np.array([1e-3, 2e-3, 5e-4])}
CYCLES, SCALING = 2, 0.1
_REF = {}


def _w0(n=N, b=B):
    return np.random.default_rng(5).standard_normal((b, n, n)).astype(np.float32)


def _random_amplitudes(numpy_seed, device):
    """The 6 x cycles uniform draws per sample that the solver makes after np.random.seed(numpy_seed): one numpy draw seeds a torch
    generator on the device, which is asked for [B, 1, 1] uniforms term by term."""
    np.random.seed(numpy_seed)
    gen = torch.Generator(device)
    gen.manual_seed(int(np.random.randint(1, 1000000000)))
    a = [torch.rand(B, 1, 1, generator=gen, device=device).reshape(B).cpu().numpy() for _ in range(6 * CYCLES)]
    return np.asarray(a, np.float64).reshape(CYCLES, 6, B)


def _reference(force, visc, amplitudes=None):
    """(float64 snapshots, float32 snapshots, force field) of the oracle; computed once per case."""
    key = (force, visc, None if amplitudes is None else amplitudes.tobytes())
    if key not in _REF:
        f = oracle.force_field(force, B, N, torch.float64, amplitudes, CYCLES, SCALING)
        f64 = None if f is None else f.numpy()
        r64 = oracle.solve(_w0(), VISC[visc], STEPS, DT, STEPS // RECORDS, f64, torch.float64)
        r32 = oracle.solve(_w0(), VISC[visc], STEPS, DT, STEPS // RECORDS, f64, torch.float32)
        assert oracle.rel_l2(r64[..., -1], _w0()) > 1e-2      # the flow moves: a solver that does nothing cannot pass
        _REF[key] = (r64, r32, f64)
    return _REF[key]


@pytest.mark.parametrize("visc", ["scalar", "array"])
@pytest.mark.parametrize("force", ["li", "kolmogorov", "none", "random"])
def test_solver_follows_the_float64_oracle(host_device, force, visc):
    amplitudes = _random_amplitudes(77, host_device) if force == "random" else None
    r64, r32, f64 = _reference(force, visc, amplitudes)
    np.random.seed(77)
    sol, f = solve_navier_stokes_2d(torch.from_numpy(_w0()).to(host_device), VISC[visc], STEPS * DT, DT, RECORDS, CYCLES, SCALING,
                                    0.2, Force(force), False)
    assert isinstance(sol, np.ndarray) and sol.shape == (B, N, N, RECORDS) and sol.dtype == np.float32
    if force == "none":
        assert f is None
    else:
        assert isinstance(f, np.ndarray) and f.shape == ((B, N, N) if force == "random" else (N, N))
        # the fp32 grid coordinate times up to 8 pi carries half an ulp of 25 (1e-6) into the argument of sin / cos
        assert oracle.rel_l2(f, f64) <= 2e-6
    bound = max(1e-5, 4 * oracle.rel_l2(r32, r64))
    errs = [oracle.rel_l2(sol[..., i], r64[..., i]) for i in range(RECORDS)]
    print(f"[ns2d {force} visc={visc}] float32 oracle {oracle.rel_l2(r32, r64):.2e}, solver " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= bound, (errs, bound)


def test_recording_follows_record_time(host_device):
    """record_time = floor(steps / record_steps): 10 steps, 3 snapshots -> every 3rd step (steps 3, 6, 9)."""
    r64 = oracle.solve(_w0(), 1e-3, 9, DT, 3, None, torch.float64)
    sol, _ = solve_navier_stokes_2d(torch.from_numpy(_w0()).to(host_device), 1e-3, STEPS * DT, DT, 3, force=Force.none)
    assert sol.shape == (B, N, N, 3)
    assert oracle.rel_l2(sol, r64) <= 1e-5


def test_gaussian_rf_is_the_oracle_on_the_same_draw(host_device):
    grf = GaussianRF(2, N, alpha=2.5, tau=7, device=host_device)
    torch.manual_seed(3)
    u = grf.sample(4)
    torch.manual_seed(3)
    noise = torch.randn(4, N, N, 2, device=host_device)
    assert u.shape == (4, N, N) and u.dtype == torch.float32 and str(u.device) == str(torch.device(host_device))
    assert oracle.rel_l2(u.cpu().numpy(), oracle.gaussian_rf(noise.cpu().numpy(), 2.5, 7)) <= 1e-5
    grf = GaussianRF(2, N, alpha=2, tau=3, sigma=0.5, device=host_device)
    torch.manual_seed(4)
    u = grf.sample(2)
    torch.manual_seed(4)
    noise = torch.randn(2, N, N, 2, device=host_device)
    assert oracle.rel_l2(u.cpu().numpy(), oracle.gaussian_rf(noise.cpu().numpy(), 2, 3, 0.5)) <= 1e-5
    for n_dims in (1, 3):
        with pytest.raises(NotImplementedError):
            GaussianRF(n_dims, N)


def test_solver_refusals(host_device):
    w0 = torch.from_numpy(_w0()).to(host_device)
    with pytest.raises(NotImplementedError, match="varying_force"):
        solve_navier_stokes_2d(w0, 1e-3, 0.1, DT, 5, CYCLES, SCALING, 0.2, Force.random, True)
    for n in (12, 4):      # not a power of two; below the smallest grid
        with pytest.raises(ValueError, match="power of two"):
            solve_navier_stokes_2d(torch.zeros(B, n, n, device=host_device), 1e-3, 0.1, DT, 5)
    with pytest.raises(ValueError, match="visc"):
        solve_navier_stokes_2d(w0, np.array([1e-3, 1e-3]), 0.1, DT, 5)
    with pytest.raises(ValueError, match=r"\[B, N, N\]"):
        solve_navier_stokes_2d(w0[:, :, :8], 1e-3, 0.1, DT, 5)


def test_nan_is_reported(host_device):
    w0 = torch.from_numpy(_w0()).to(host_device)
    w0[0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        solve_navier_stokes_2d(w0, 1e-3, 0.1, DT, 5, force=Force.none)


@pytest.mark.gpu
def test_solver_at_the_generator_grid():
    """N = 256 (the generator's default grid, many workgroups per launch), B = 2, 5 steps of 1e-3 with the `li` force."""
    n, b, steps, dt = 256, 2, 5, 1e-3
    w0 = _w0(n, b)
    f = oracle.force_field("li", b, n, torch.float64).numpy()
    visc = np.array([1e-3, 1e-4])
    r64 = oracle.solve(w0, visc, steps, dt, steps, f, torch.float64)
    r32 = oracle.solve(w0, visc, steps, dt, steps, f, torch.float32)
    assert oracle.rel_l2(r64[..., -1], w0) > 1e-2
    sol, _ = solve_navier_stokes_2d(torch.from_numpy(w0).to("cuda:0"), visc, steps * dt, dt, 1, force=Force.li)
    e, e32 = oracle.rel_l2(sol[..., 0], r64[..., 0]), oracle.rel_l2(r32, r64)
    print(f"[ns2d N=256] float32 oracle {e32:.2e}, solver {e:.2e}")
    assert e <= max(1e-5, 4 * e32)
