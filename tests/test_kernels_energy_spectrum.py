"""ffno_energy_spectrum (include/ffno.h, csrc/ffno_pred_export.h) through the C ABI, on the emulator and on the GPU, against a
float64 numpy restatement of the definition in include/ffno.h -- which is itself pinned by closed forms first: a plane wave, the
integer shell rule against floor(|k| + 1/2), Parseval.

Bound on E[s] (u = 2^-24, first order).  All terms are non-negative, so the bound is RELATIVE to E[s].  A term
h ((re^2 + im^2) + (re^2 + im^2)) carries a product, an inner and the outer addition: 3 u (h = 1 or 2 is exact).  The summation
order is fixed (include/ffno.h): lane l of one wave adds the shell's bins of rows l, l + 64, ... sequentially -- n - 1 roundings
for its n terms -- then six butterfly additions, then the product with 1 / (2 m^4), itself rounded to fp32: 2 u.  Together
(n - 1 + 3 + 6 + 2) u = (n + 10) u with n the most terms any lane holds in that shell, which `_lane_terms` counts from the
definition; the test allows (n + 11) u, one u for the second-order terms.  The oracle reads the very fp32 spectra the kernel
reads, so no input error enters.
"""
import numpy as np
import pytest

from backend_util import be  # noqa: F401

U = 2.0 ** -24


def _shells(m):
    """[m][m/2+1] integer shell of every bin of a half spectrum, by the integer inequalities of include/ffno.h."""
    r, c = np.meshgrid(np.arange(m), np.arange(m // 2 + 1), indexing="ij")
    kx = np.where(r < m // 2, r, r - m)
    k2x4 = 4 * (kx * kx + c * c)
    s = np.zeros_like(k2x4)
    while True:      # the shell is the largest s with (2 s - 1)^2 <= 4 k^2 (s = 0 takes what is left)
        up = (2 * (s + 1) - 1) ** 2 <= k2x4
        if not up.any():
            return s
        s = s + up


def spectrum64(u_h, v_h, corners=False):
    """u_h, v_h [..., m, m/2+1] complex -> E [..., m/2+1] in float64 (with `corners`: every shell up to the largest)."""
    u_h, v_h = np.asarray(u_h, np.complex128), np.asarray(v_h, np.complex128)
    m = u_h.shape[-2]
    s = _shells(m)
    h = np.full(m // 2 + 1, 2.0)
    h[0] = h[m // 2] = 1.0
    e = h * (np.abs(u_h) ** 2 + np.abs(v_h) ** 2) / (2.0 * float(m) ** 4)
    n = s.max() + 1 if corners else m // 2 + 1
    out = np.zeros(u_h.shape[:-2] + (n,))
    for k in range(n):
        out[..., k] = (e * (s == k)).sum(axis=(-2, -1))
    return out


def _lane_terms(m):
    """[m/2+1]: the most bins of shell s that one lane adds (lane l holds rows l, l + 64, l + 128, l + 192)."""
    s = _shells(m)
    out = np.zeros(m // 2 + 1, int)
    for k in range(m // 2 + 1):
        per_row = (s == k).sum(axis=1)
        out[k] = max(per_row[l::64].sum() for l in range(min(m, 64)))
    return out


# ---- the oracle against known answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1, 0), (0, 2), (3, 4), (-2, 3), (6, 5), (7, 0), (-5, -6)])
def test_oracle_plane_wave_puts_a_quarter_of_the_squared_amplitude_in_one_shell(a, b):
    m, A = 16, 1.7
    x = 2 * np.pi * np.arange(m) / m
    u = A * np.cos(a * x[:, None] + b * x[None, :])
    E = spectrum64(np.fft.rfft2(u), np.zeros((m, m // 2 + 1)))
    want = np.zeros(m // 2 + 1)
    want[int(round(np.sqrt(a * a + b * b)))] = A * A / 4
    np.testing.assert_allclose(E, want, atol=1e-13)


def test_oracle_leaves_a_corner_wave_out():
    m = 16
    x = 2 * np.pi * np.arange(m) / m
    u_h = np.fft.rfft2(np.cos(7 * x[:, None] + 7 * x[None, :]))      # |k| = 9.9: shell 10 > m / 2
    z = np.zeros_like(u_h)
    assert np.abs(spectrum64(u_h, z)).max() < 1e-13
    full = spectrum64(u_h, z, corners=True)
    assert abs(full[10] - 0.25) < 1e-13 and abs(full.sum() - 0.25) < 1e-13


def test_integer_shell_rule_is_the_rounded_distance_for_every_bin_of_64():
    """(2 s + 1)^2 is odd and 4 k^2 even: no bin lies at distance exactly s + 1/2, so the integer rule and the rounded float64
    square root (exact to half an ulp, far less than the gap of 1 / (4 |k|) to the nearest half-integer) must agree everywhere."""
    m = 64
    r, c = np.meshgrid(np.arange(m), np.arange(m // 2 + 1), indexing="ij")
    kx = np.where(r < m // 2, r, r - m)
    k2 = (kx * kx + c * c).astype(np.float64)
    s = _shells(m)
    assert np.array_equal(s, np.floor(np.sqrt(k2) + 0.5).astype(int))
    assert ((2 * s - 1) ** 2 <= 4 * k2)[s > 0].all() and (4 * k2 < (2 * s + 1) ** 2).all()
    assert s[0, 0] == 0 and (s == 0).sum() == 1 and s.max() == 45      # sqrt(2) 32 = 45.25


@pytest.mark.parametrize("m", [8, 16, 64])
def test_oracle_parseval_with_the_corner_shells_added_back(m):
    rs = np.random.RandomState(m)
    u, v = rs.standard_normal((2, m, m)) + 0.4
    E = spectrum64(np.fft.rfft2(u), np.fft.rfft2(v), corners=True)
    assert abs(E.sum() - ((u * u + v * v) / 2).mean()) < 1e-12
    assert E[m // 2 + 1:].sum() > 0.05      # the corners hold a real share of white noise: leaving them out is a decision


# ---- the kernel against the oracle -----------------------------------------------------------------------------------------
def _fields(m, n_img=3):
    rs = np.random.RandomState(1000 + m)
    u, v = rs.standard_normal((2, n_img, m, m)) + 0.3
    return np.fft.rfft2(u).astype(np.complex64), np.fft.rfft2(v).astype(np.complex64)


def _run(be, u_h, v_h):
    lib, p = be.lib, be.ptr
    n_img, m = u_h.shape[0], u_h.shape[1]
    E = be.empty((n_img, m // 2 + 1))
    pair = lambda z: be.put(np.ascontiguousarray(z).view(np.float32).reshape(*z.shape, 2))      # noqa: E731
    assert lib.ffno_energy_spectrum(p(pair(u_h)), p(pair(v_h)), p(E), n_img, m, None) == 0
    return be.get(E).copy()


@pytest.mark.parametrize("m", [8, 16, 64])
def test_energy_spectrum_matches_float64_and_two_runs_give_the_same_bits(be, m):
    u_h, v_h = _fields(m)
    got = _run(be, u_h, v_h)
    want = spectrum64(u_h, v_h)
    assert got.shape == want.shape == (3, m // 2 + 1) and (want > 0).all()
    rel = np.abs(got.astype(np.float64) - want) / want
    bound = (_lane_terms(m) + 11) * U
    print(f"m={m}: max rel err / bound {np.max(rel / bound):.3f}; largest rel err {rel.max():.3e}, lane terms up to {_lane_terms(m).max()}")
    assert (rel <= bound).all()
    assert _run(be, u_h, v_h).tobytes() == got.tobytes()


def test_energy_spectrum_of_a_plane_wave_on_the_device(be):
    """One bin pair per image: every other shell is exactly zero."""
    m, A = 16, 1.5
    x = 2 * np.pi * np.arange(m) / m
    waves = [(3, 4), (0, 2), (7, 7)]
    u = np.stack([A * np.cos(a * x[:, None] + b * x[None, :]) for a, b in waves])
    u_h = np.fft.rfft2(u).astype(np.complex64)
    got = _run(be, u_h, np.zeros_like(u_h)).astype(np.float64)
    want = spectrum64(u_h, np.zeros_like(u_h))
    assert abs(want[0, 5] - A * A / 4) < 1e-6 and abs(want[1, 2] - A * A / 4) < 1e-6 and want[2].max() < 1e-12
    assert np.abs(got - want).max() <= 12 * U * A * A / 4


def test_energy_spectrum_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    a, E = be.zeros((16 * 9 * 2,)), be.zeros((9,))
    assert lib.ffno_energy_spectrum(p(a), p(a), p(E), 1, 16, None) == 0
    for m in (6, 12, 7, 512):
        assert lib.ffno_energy_spectrum(p(a), p(a), p(E), 1, m, None) == -2
    assert lib.ffno_energy_spectrum(None, p(a), p(E), 1, 16, None) == -1
    assert lib.ffno_energy_spectrum(p(a), None, p(E), 1, 16, None) == -1
    assert lib.ffno_energy_spectrum(p(a), p(a), None, 1, 16, None) == -1
    assert lib.ffno_energy_spectrum(p(a), p(a), p(E), 0, 16, None) == -1
    assert lib.ffno_energy_spectrum(p(a), p(a), p(E), 1, 0, None) == -1
