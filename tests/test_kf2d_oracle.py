"""tests/kf2d_oracle.py, the float64 restatement the Kolmogorov-flow kernels and solver are compared with, is itself pinned here on
the CPU by what the equation and the scheme promise: the decay rate of a single mode, the orders of the explicit part (4) and of
the whole step (2, Crank-Nicolson), and the laminar Kolmogorov state as a fixed point."""
import numpy as np

import kf2d_oracle as oracle

N = 16


def _grid(N):
    x = (np.arange(N) + 0.5) * 2 * np.pi / N
    return x[:, None], x[None, :]


def _order(errors):
    return [float(np.log2(a / b)) for a, b in zip(errors, errors[1:])]


def test_single_mode_decays_at_the_linear_rate():
    """w = cos(2 x + 3 y) advects nothing (v . grad w = 0 for one mode), so w(t) = w(0) exp(-(nu |k|^2 + drag) t); the error of the
    Crank-Nicolson part falls by about 4 x per halving of dt."""
    X, Y = _grid(N)
    w0 = np.cos(2 * X + 3 * Y)
    nu, drag, T = 0.05, 0.1, 1.0
    want = w0 * np.exp(-(nu * 13 + drag) * T)
    errs = []
    for n in (8, 16, 32):
        errs.append(oracle.rel_l2(oracle.Solver(N, nu, drag, T / n).run(w0, n), want))
    print(f"[kf2d oracle decay] errors {errs}, orders {_order(errs)}")
    assert errs[-1] < 1e-4
    assert all(3.5 <= a / b <= 4.5 for a, b in zip(errs, errs[1:])), errs


def _two_modes():
    X, Y = _grid(N)
    return np.cos(X + 2 * Y) + 0.7 * np.sin(2 * X - Y) + 0.5 * np.cos(Y)


def _errors(solver_of, T, ns, finer=16):
    w0 = _two_modes()
    fine = solver_of(T / (ns[-1] * finer)).run(w0, ns[-1] * finer)
    moved = oracle.rel_l2(fine, w0)
    assert moved > 1e-2, moved      # the flow does something over T
    return [oracle.rel_l2(solver_of(T / n).run(w0, n), fine) for n in ns]


def test_explicit_part_is_fourth_order():
    errs = _errors(lambda dt: oracle.Solver(N, 0.0, 0.0, dt, wavenumber=4, magnitude=1.0, linear_coefficient=-0.1), 1.0, (8, 16, 32))
    print(f"[kf2d oracle explicit] errors {errs}, orders {_order(errs)}")
    assert min(_order(errs)) >= 3.5, (errs, _order(errs))


def test_whole_step_is_second_order():
    errs = _errors(lambda dt: oracle.Solver(N, 0.05, 0.1, dt, wavenumber=4, magnitude=1.0), 1.0, (8, 16, 32))
    print(f"[kf2d oracle whole step] errors {errs}, orders {_order(errs)}")
    assert min(_order(errs)) >= 1.8, (errs, _order(errs))


def test_laminar_state_is_a_fixed_point():
    """w* = -k_f cos(k_f y_j) / (nu k_f^2 + drag) balances forcing, viscosity and drag, and a parallel shear flow advects nothing."""
    nu, drag, kf = 1e-3, 0.1, 4
    f = oracle.force_field(N, kf, 1.0)
    w_star = f / (nu * kf ** 2 + drag)
    dt = 0.5 * (2 * np.pi / N) / 7.0
    got = oracle.Solver(N, nu, drag, dt, wavenumber=kf, magnitude=1.0).run(w_star, 50)
    drift = oracle.rel_l2(got, w_star)
    print(f"[kf2d oracle laminar] drift {drift:.2e}")
    assert drift < 1e-6


def test_forcing_spectrum_is_one_bin_of_the_half_spectrum():
    """f_h(0, k_f) = -magnitude k_f (N^2 / 2) e^{i k_f pi / N}, every other bin of rfft2 zero: what the stage kernel is handed."""
    for n, kf, mag in ((16, 4, 1.0), (32, 2, 0.5)):
        f_h = np.fft.rfft2(oracle.force_field(n, kf, mag))
        want = np.zeros_like(f_h)
        want[0, kf] = -mag * kf * (n * n / 2) * np.exp(1j * kf * np.pi / n)
        np.testing.assert_allclose(f_h, want, atol=1e-9 * n * n)


def test_downsample_of_the_oracle_is_the_coarse_curl():
    """On a band-limited field the reduced vorticity tends to the field itself at the coarse cell centres' staggered positions;
    here only the identity case and the shape are pinned -- the formulas are tests/coarsen_oracle.py's, pinned in
    test_kernels_coarsen.py."""
    w = _two_modes()
    s = oracle.Solver(N, 1e-3, 0.1, 1e-2)
    assert np.array_equal(s.downsample(w, N), w)
    assert s.downsample(w, 8).shape == (8, 8) and abs(s.downsample(w, 8).mean()) < 1e-12
