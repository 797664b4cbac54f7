"""KolmogorovStepper and initial_vorticity (fourierflow_amd/builders/kolmogorov_flow.py) on the emulator and on an MI355X against
the float64 restatement tests/kf2d_oracle.py, which runs the step in its full complex FFT form: N = 16, B = 3, 20 steps at the
time step of stable_time_step, the shipped re_1000 physics (viscosity 1e-3, drag 0.1, forcing wavenumber 4).  Bound 1e-5 per
compared field, the bound of test_ns2d_golden.py for 10 steps of that solver; the fp32 restatement of the same formulas would
sit at a few 1e-7."""
import numpy as np
import pytest
import torch

import kf2d_oracle as oracle
from backend_util import host_device  # noqa: F401

N, B, STEPS = 16, 3, 20
NU, DRAG, KF, MAG = 1e-3, 0.1, 4, 1.0
MAX_V, KP, SEED = 7.0, 4.0, 73714
BOUND = 1e-5
_CACHE = {}


def _dt():
    from fourierflow_amd.builders import stable_time_step
    return stable_time_step(MAX_V, 0.5, NU, 2 * np.pi / N)


def _w0():
    from fourierflow_amd.builders import initial_vorticity
    if "w0" not in _CACHE:
        _CACHE["w0"] = initial_vorticity(B, N, MAX_V, KP, SEED).numpy()
    return _CACHE["w0"]


def _reference(c):
    """The oracle's final field for linear coefficient c, computed once per session."""
    if c not in _CACHE:
        _CACHE[c] = oracle.Solver(N, NU, DRAG, _dt(), KF, MAG, c).run(_w0(), STEPS)
    return _CACHE[c]


def test_stable_time_step_is_the_advective_limit_here():
    assert _dt() == pytest.approx(0.5 * (2 * np.pi / N) / MAX_V, rel=1e-15)
    from fourierflow_amd.builders import stable_time_step
    assert stable_time_step(7.0, 0.5, 1e-3, 2 * np.pi / 2048) == pytest.approx(0.0002191401125550916, rel=1e-12)
    assert stable_time_step(1e-3, 0.5, 1.0, 0.1) == pytest.approx(0.1 ** 2 / 4, rel=1e-15)      # the diffusive limit


@pytest.mark.parametrize("c", [0.0, -0.1])
def test_twenty_steps_match_the_float64_oracle(host_device, c):
    from fourierflow_amd.builders import KolmogorovStepper
    w0, want = _w0(), _reference(c)
    moved = oracle.rel_l2(want, w0)
    assert moved > 1e-2, moved      # the flow moved: the comparison is not of two copies of w0
    st = KolmogorovStepper(torch.from_numpy(w0).to(host_device), NU, DRAG, _dt(), KF, MAG, c)
    for _ in range(STEPS):
        st.step()
    got = st.vorticity().cpu().numpy()
    e = oracle.rel_l2(got, want)
    sol = oracle.Solver(N, NU, DRAG, _dt(), KF, MAG, c)
    e8 = oracle.rel_l2(st.downsample(8).cpu().numpy(), sol.downsample(want, 8))
    e16 = oracle.rel_l2(st.downsample(16).cpu().numpy(), want)
    print(f"[kf2d solver c={c}] moved {moved:.2e}, vorticity {e:.2e}, downsample(8) {e8:.2e}, downsample(16) {e16:.2e}")
    assert e <= BOUND and e8 <= BOUND and e16 <= BOUND
    vel = st.velocity().cpu().numpy()
    vx, vy = sol.velocity(np.fft.fft2(want))
    assert oracle.rel_l2(vel[0], vx) <= BOUND and oracle.rel_l2(vel[1], vy) <= BOUND


def test_laminar_state_stays_put_on_the_kernels(host_device):
    """The fixed point of the oracle test, through the kernels in fp32: the forced bin balances viscosity and drag."""
    from fourierflow_amd.builders import KolmogorovStepper
    w_star = oracle.force_field(N, KF, MAG) / (NU * KF ** 2 + DRAG)
    st = KolmogorovStepper(torch.from_numpy(np.tile(w_star, (B, 1, 1)).astype(np.float32)).to(host_device), NU, DRAG, _dt(), KF, MAG)
    for _ in range(STEPS):
        st.step()
    drift = oracle.rel_l2(st.vorticity().cpu().numpy()[1], w_star)
    print(f"[kf2d solver laminar] drift {drift:.2e}")
    assert drift <= BOUND


def test_stepper_on_the_doubled_domain(host_device):
    """[0, 4 pi)^2 as in the large_domain files: forcing wavenumber 4 is bin 8 there."""
    from fourierflow_amd.builders import KolmogorovStepper, initial_vorticity
    n, L = 32, 4 * np.pi
    dt = 0.5 * (L / n) / MAX_V
    w0 = initial_vorticity(2, n, MAX_V, KP, SEED, length=L).numpy()
    sol = oracle.Solver(n, NU, DRAG, dt, KF, MAG, length=L)
    want = sol.run(w0, 10)
    assert oracle.rel_l2(want, w0) > 1e-2
    st = KolmogorovStepper(torch.from_numpy(w0).to(host_device), NU, DRAG, dt, KF, MAG, length=L)
    assert st.kf == 8
    for _ in range(10):
        st.step()
    e = oracle.rel_l2(st.vorticity().cpu().numpy(), want)
    e8 = oracle.rel_l2(st.downsample(8).cpu().numpy(), sol.downsample(want, 8, L))
    print(f"[kf2d solver 4 pi] vorticity {e:.2e}, downsample(8) {e8:.2e}")
    assert e <= BOUND and e8 <= BOUND


def test_stepper_refuses_what_the_kernels_do_not_cover(host_device):
    from fourierflow_amd.builders import KolmogorovStepper
    with pytest.raises(ValueError, match="16 ... 4096"):
        KolmogorovStepper(torch.zeros(1, 24, 24, device=host_device), NU, DRAG, 1e-2)
    with pytest.raises(ValueError, match="whole number"):
        KolmogorovStepper(torch.zeros(1, 16, 16, device=host_device), NU, DRAG, 1e-2, 8, 1.0)      # bin 8 = N/2
    st = KolmogorovStepper(torch.zeros(1, 16, 16, device=host_device), NU, DRAG, 1e-2)
    with pytest.raises(ValueError, match="does not divide"):
        st.downsample(6)


def _speed_max(w, length=2 * np.pi):
    vx, vy = oracle.Solver(w.shape[-1], 0, 0, 1.0, length=length).velocity(np.fft.fft2(w.astype(np.float64)))
    return np.sqrt(vx ** 2 + vy ** 2).reshape(len(w), -1).max(axis=1)


def test_initial_vorticity_scale_mean_and_batch_independence():
    from fourierflow_amd.builders import initial_vorticity
    w = _w0()
    assert w.dtype == np.float32 and w.shape == (B, N, N)
    np.testing.assert_allclose(_speed_max(w), MAX_V, rtol=1e-5)
    assert np.abs(w.astype(np.float64).mean(axis=(1, 2))).max() <= 1e-6 * np.abs(w).max()
    singles = np.concatenate([initial_vorticity(1, N, MAX_V, KP, SEED, first_index=i).numpy() for i in range(B)])
    np.testing.assert_array_equal(singles, w)      # sample i is the same field in a batch of 1 and in a batch of 3
    assert not np.array_equal(w[0], w[1])
    assert not np.array_equal(initial_vorticity(1, N, MAX_V, KP, SEED + 1).numpy()[0], w[0])


def test_initial_vorticity_spectrum_peaks_at_the_peak_wavenumber():
    """E(k) ~ k^4 exp(-2 (k / k_p)^2): over 64 samples at N = 64 the shell-summed energy of the velocity has its maximum in the
    shell k_p = 4 (the neighbouring shells carry 0.76 and 0.79 of it in the continuum; 64 samples of ~25 modes leave ~3% noise),
    and with k_p = 6 in shell 6."""
    from fourierflow_amd.builders import initial_vorticity
    n = 64
    i = np.fft.fftfreq(n, 1.0 / n)
    k = np.sqrt(i[:, None] ** 2 + i[None, :] ** 2)
    for kp in (4.0, 6.0):
        w = initial_vorticity(64, n, MAX_V, kp, 5).numpy().astype(np.float64)
        mode_energy = (np.abs(np.fft.fft2(w)) ** 2 / np.where(k > 0, k, 1.0) ** 2).mean(axis=0)      # |u_h|^2 = |w_h|^2 / k^2
        shells = np.array([mode_energy[(k >= s - 0.5) & (k < s + 0.5)].sum() for s in range(1, n // 3)])
        print(f"[kf2d initial k_p={kp}] shells {np.round(shells / shells.max(), 3)[:10]}")
        assert 1 + int(np.argmax(shells)) == int(kp)
