"""ffno_vorticity_coarsen_step / ffno_vorticity_coarsen_ws_floats / ffno_markov_corr_metrics (include/ffno.h,
csrc/ffno_coarsen.h; reference utils/array.py:18-80, routines/grid_2d_markov.py:350-370) through the C ABI, on the emulator and
on the GPU, against the float64 restatement of tests/coarsen_oracle.py -- which is itself pinned by a closed form first.

Bound on w_c (absolute, u = 2^-24, first order).  The kernel's mean is a sequential fp32 sum of f terms in index order, then one
division by f: the sum carries at most (f - 1) u sum|x| <= (f - 1) f u max|x|, the division adds u |mean|, so
|d u_c| <= f u max|u| and |d v_c| <= f u max|v|.  A = (v_c[i+1] - v_c[i]) / dx then carries 2 f u max|v| / dx inherited, and
u |A| <= 2 u max|v| / dx three times over: the subtraction, the fp32 rounding of dx = len_x / m, the division.  The same for
B = (u_c[j+1] - u_c[j]) / dy.  The final A - B rounds once more, u |w_c| <= 2 u (max|v| / dx + max|u| / dy).  Together
(2 f + 8) u (max|v| / dx + max|u| / dy) <= 6 f u (...) for f >= 2; the test allows c = 8 in  c f 2^-24 (max|v| / dx + max|u| / dy),
which leaves room for the second-order terms and a division done through a reciprocal.

Bound on the sums.  A per-sample sum adds n = m m products: a thread's fma chain of ceil(n / (256 S)) terms, the butterfly of
a wave, four waves, S slices -- as in tests/test_kernels_markov_traj.py at most (ceil(log2 n) + 3) 2^-24 of the sum of the terms'
magnitudes; n <= 1600 here gives 14 * 2^-24 = 8.4e-7, and 2e-6 is kept.  The two sums of squares are held to it RELATIVELY; for
sum w_c c the magnitudes add up to at most sqrt(sum w_c^2 sum c^2) (Cauchy-Schwarz), which scales the absolute bound.  The sums
are compared with float64 arithmetic on the fp32 w_c that the same launch wrote into preds2, so the bound is the summation's
alone.
"""
import numpy as np
import pytest

import coarsen_oracle as co
from backend_util import be  # noqa: F401

NS = 3
U = 2.0 ** -24
TWO_PI = 2 * np.pi


# ---- the oracle against a known answer ----------------------------------------------------------------------------------
def _block_mean_sin(theta, delta, f):
    """mean_{k<f} sin(theta + k delta) = sin(theta + (f - 1) delta / 2) sin(f delta / 2) / (f sin(delta / 2))."""
    if abs(np.sin(delta / 2)) < 1e-14:      # delta a multiple of 2 pi: every term is sin(theta)
        return np.sin(theta)
    return np.sin(theta + (f - 1) * delta / 2) * np.sin(f * delta / 2) / (f * np.sin(delta / 2))


@pytest.mark.parametrize("X,m", [(24, 8), (32, 8), (16, 8)])
@pytest.mark.parametrize("a,b", [(1, 0), (0, 2), (3, 5), (2, -3)])
def test_oracle_plane_wave_known_answer(a, b, X, m):
    """w = cos(a x + b y) on [0, 2 pi)^2: u = -b sin(.) / (a^2 + b^2), v = a sin(.) / (a^2 + b^2) (tests/test_velocity.py); the
    block means of a sinusoid are closed forms, and so is w_c: the closed forms are evaluated at i + 1 and j + 1 themselves, past
    the last index too, so that the oracle's periodic wrap is checked against the function's own periodicity."""
    f, k2, h = X // m, a * a + b * b, TWO_PI / X
    x = np.arange(X) * h
    w = np.cos(a * x[:, None] + b * x[None, :])
    u, v = co.velocity(w)
    np.testing.assert_allclose(u, -b * np.sin(a * x[:, None] + b * x[None, :]) / k2, atol=1e-12)
    np.testing.assert_allclose(v, a * np.sin(a * x[:, None] + b * x[None, :]) / k2, atol=1e-12)

    def u_c(i, j):      # line f i + f - 1 along x, the mean over y = f j ... f j + f - 1
        return -b / k2 * _block_mean_sin(a * h * (f * i + f - 1) + b * h * f * j, b * h, f)

    def v_c(i, j):      # line f j + f - 1 along y, the mean over x = f i ... f i + f - 1
        return a / k2 * _block_mean_sin(a * h * f * i + b * h * (f * j + f - 1), a * h, f)

    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    got_u, got_v = co.coarsen_velocity(u, v, m)
    np.testing.assert_allclose(got_u, u_c(i, j), atol=1e-12)
    np.testing.assert_allclose(got_v, v_c(i, j), atol=1e-12)
    d = TWO_PI / m
    want = (v_c(i + 1, j) - v_c(i, j)) / d - (u_c(i, j + 1) - u_c(i, j)) / d
    np.testing.assert_allclose(co.curl(got_u, got_v), want, atol=1e-12)
    np.testing.assert_allclose(co.downsample_vorticity(w[None, :, :, None], m)[0, :, :, 0], want, atol=1e-12)
    np.testing.assert_allclose(co.coarsen_from_velocity(np.stack([w, u, v], axis=-1), m), want, atol=1e-12)


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------
def _slices(lib, B, m, n_steps):
    ws = int(lib.ffno_vorticity_coarsen_ws_floats(B, m, n_steps))
    assert ws > 0 and ws % (n_steps * B * NS) == 0
    return ws, ws // (n_steps * B * NS)


def _case(seed, B, X, m, Tc):
    """Random fields with an offset and a ramp: nothing periodic about them, so a missing wrap or the wrong line of a block shows."""
    rs = np.random.RandomState(seed)
    ramp = np.linspace(-1.0, 2.0, X)
    vel = rs.standard_normal((B, X, X, 3)) + 0.3 + ramp[None, :, None, None] - 0.5 * ramp[None, None, :, None]
    corr = rs.standard_normal((B, m, m, Tc)) + 0.2
    return vel.astype(np.float32), corr.astype(np.float32)


def _run(be, vel, corr, n_steps, t, lx, ly, with_preds=True):
    lib, p = be.lib, be.ptr
    B, X, Y, _ = vel.shape
    m, Tc = corr.shape[1], corr.shape[3]
    ws, S = _slices(lib, B, m, n_steps)
    d_preds, d_sums = be.empty((B, m, m, n_steps)), be.empty((ws,))
    rc = lib.ffno_vorticity_coarsen_step(p(be.put(vel)), p(be.put(corr)), p(d_preds) if with_preds else None, p(d_sums), B, X, Y, m,
                                         Tc, n_steps, t, lx, ly, None)
    assert rc == 0
    return be.get(d_preds).copy(), be.get(d_sums).copy().reshape(n_steps, B, S, NS), S


def _check(be, vel, corr, n_steps, t, lx, ly, slices):
    B, X = vel.shape[:2]
    m, Tc = corr.shape[1], corr.shape[3]
    f = X // m
    preds, sums, S = _run(be, vel, corr, n_steps, t, lx, ly)
    assert S == slices
    lx64, ly64 = float(np.float32(lx)), float(np.float32(ly))      # the lengths as the C ABI takes them
    want = co.coarsen_from_velocity(vel, m, lx64, ly64)
    bound = 8 * f * U * (np.abs(vel[..., 2]).max() / (lx64 / m) + np.abs(vel[..., 1]).max() / (ly64 / m))
    err = np.abs(preds[..., t].astype(np.float64) - want).max()
    print(f"X={X} m={m} f={f} t={t}: max |w_c - float64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    other = [k for k in range(n_steps) if k != t]
    assert np.isnan(preds[..., other]).all() and np.isnan(sums[other]).all()      # one step writes its own column only
    w6, c6 = preds[..., t].astype(np.float64), corr[..., Tc - n_steps + t].astype(np.float64)
    got = sums[t].astype(np.float64).sum(axis=1)
    ww, cc, wc = (w6 ** 2).sum((1, 2)), (c6 ** 2).sum((1, 2)), (w6 * c6).sum((1, 2))
    errs = np.abs(got[:, 0] - ww) / ww, np.abs(got[:, 1] - cc) / cc, np.abs(got[:, 2] - wc) / np.sqrt(ww * cc)
    print("sums: max rel err %.3e %.3e, max err / sqrt(sum w^2 sum c^2) %.3e" % tuple(e.max() for e in errs))
    assert max(e.max() for e in errs) < 2e-6
    if S > 1:
        assert (sums[t][:, :, 1] > 0).all()      # every slice carries its own share
    return preds, sums


@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("X,m", [(16, 8), (32, 8), (64, 8), (24, 8)])
def test_coarsen_step_matches_float64(be, X, m, t):
    vel, corr = _case(100 + X, 3, X, m, 5)
    _check(be, vel, corr, 3, t, TWO_PI, TWO_PI, slices=1)


def test_coarsen_step_with_unequal_domain_lengths(be):
    vel, corr = _case(7, 3, 32, 8, 5)
    preds, _ = _check(be, vel, corr, 3, 2, 1.0, 3.0, slices=1)
    same = co.coarsen_from_velocity(vel, 8, 3.0, 1.0)      # the two lengths exchanged: far outside the bound
    assert np.abs(preds[..., 2] - same).max() > 1e-2


def test_coarsen_step_several_slices_per_sample(be):
    """m = 40: 1600 cells in two slices of 20 coarse rows; the halo row of slice 0 is slice 1's first, that of slice 1 wraps."""
    vel, corr = _case(8, 3, 80, 40, 5)
    _check(be, vel, corr, 3, 1, TWO_PI, TWO_PI, slices=2)


def test_coarsen_step_without_preds_writes_the_same_sums_and_runs_are_bit_equal(be):
    vel, corr = _case(9, 3, 32, 8, 5)
    preds, sums, _ = _run(be, vel, corr, 3, 1, TWO_PI, TWO_PI)
    preds_b, sums_b, _ = _run(be, vel, corr, 3, 1, TWO_PI, TWO_PI)
    assert np.array_equal(preds[..., 1], preds_b[..., 1]) and np.array_equal(sums[1], sums_b[1])
    none, sums_c, _ = _run(be, vel, corr, 3, 1, TWO_PI, TWO_PI, with_preds=False)
    assert np.isnan(none).all()                       # (the buffer the call did not get)
    assert np.array_equal(sums[1], sums_c[1]) and np.isnan(sums_c[[0, 2]]).all()


def test_coarsen_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    a, out = be.zeros((16 * 16 * 3,)), be.zeros((16,))

    def step(vel, corr, sums, X, Y, m, Tc, n_steps, t, lx=1.0, ly=1.0):
        return lib.ffno_vorticity_coarsen_step(vel, corr, None, sums, 1, X, Y, m, Tc, n_steps, t, lx, ly, None)

    assert step(p(a), p(a), p(out), 16, 16, 8, 3, 2, 1) == 0
    assert step(None, p(a), p(out), 16, 16, 8, 3, 2, 0) != 0
    assert step(p(a), None, p(out), 16, 16, 8, 3, 2, 0) != 0
    assert step(p(a), p(a), None, 16, 16, 8, 3, 2, 0) != 0
    assert step(p(a), p(a), p(out), 16, 16, 6, 3, 2, 0) != 0       # X % m
    assert step(p(a), p(a), p(out), 16, 12, 8, 3, 2, 0) != 0       # Y % m
    assert step(p(a), p(a), p(out), 16, 8, 4, 3, 2, 0) != 0        # X / m != Y / m
    assert step(p(a), p(a), p(out), 16, 16, 0, 3, 2, 0) != 0       # m < 1
    assert step(p(a), p(a), p(out), 16, 16, 32, 3, 2, 0) != 0      # m > X
    assert step(p(a), p(a), p(out), 16, 16, 8, 1, 2, 0) != 0       # Tc < n_steps
    assert step(p(a), p(a), p(out), 16, 16, 8, 3, 2, 2) != 0       # t >= n_steps
    assert step(p(a), p(a), p(out), 16, 16, 8, 3, 2, -1) != 0
    assert step(p(a), p(a), p(out), 16, 16, 8, 3, 2, 0, lx=0.0) != 0
    assert lib.ffno_vorticity_coarsen_ws_floats(0, 8, 2) == 0 and lib.ffno_vorticity_coarsen_ws_floats(1, 0, 2) == 0
    assert lib.ffno_markov_corr_metrics(None, p(a), 1, 8, 2, 0.95, None) != 0
    assert lib.ffno_markov_corr_metrics(p(a), p(a), 1, 0, 2, 0.95, None) != 0


# ---- the metrics -----------------------------------------------------------------------------------------------------------
def test_corr_metrics_diverge_where_the_coarse_images_part(be):
    """corr_data equal to the kernel's own coarse image for t < 2 and independent noise after: p_2 = 1 for t < 2 within the bound of
    three sums (each 2e-6 of its scale, then two square roots, a product, a division and the mean: 5e-6 holds), far below the
    threshold after, and the diverged index is exactly 2."""
    lib, p = be.lib, be.ptr
    B, X, m, Tc, n_steps = 3, 32, 8, 5, 4
    rs = np.random.RandomState(21)
    vels = [_case(30 + t, B, X, m, Tc)[0] for t in range(n_steps)]
    corr = (rs.standard_normal((B, m, m, Tc)) + 0.2).astype(np.float32)
    for t in range(2):
        corr[..., Tc - n_steps + t] = _run(be, vels[t], corr, n_steps, t, TWO_PI, TWO_PI)[0][..., t]
    ws, S = _slices(lib, B, m, n_steps)
    d_corr, d_preds, d_sums, d_m = be.put(corr), be.empty((B, m, m, n_steps)), be.empty((ws,)), be.empty((2 + n_steps,))
    for t in range(n_steps):
        assert lib.ffno_vorticity_coarsen_step(p(be.put(vels[t])), p(d_corr), p(d_preds), p(d_sums), B, X, X, m, Tc, n_steps, t,
                                               TWO_PI, TWO_PI, None) == 0
    assert lib.ffno_markov_corr_metrics(p(d_sums), p(d_m), B, m, n_steps, 0.95, None) == 0
    got = be.get(d_m).astype(np.float64)
    want, diverged = co.correlation(be.get(d_preds), corr, n_steps)
    print("p_2", got[2:], "float64 on the kernel's preds2", want)
    assert np.abs(got[2:4] - 1.0).max() < 5e-6 and np.abs(want[:2] - 1.0).max() < 1e-12
    assert np.abs(got[2:] - want).max() < 5e-6 and np.abs(want[2:]).max() < 0.9
    assert got[0] == diverged == 2
    assert abs(got[1] - want.mean()) < 5e-6
    # the threshold is an argument; the same sums, all steps above it
    assert lib.ffno_markov_corr_metrics(p(d_sums), p(d_m), B, m, n_steps, -1.0, None) == 0
    assert be.get(d_m)[0] == n_steps
