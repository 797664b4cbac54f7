"""The kernels of the Kolmogorov-flow solver step (csrc/ffno_kf2d.h: ffno_kf2d_derivs, ffno_kf2d_stage, ffno_kf2d_downsample) and
ffno_kf2d_supported through the C ABI against float64 numpy, on the emulator and on an MI355X.  Every output is a handful of fp32
roundings of its float64 value: relative L2 <= 1e-6, the bound of test_kernels_ns2d.py.  The input of derivs is a random spectrum
WITHOUT Hermitian symmetry, so the bins the kernel has to write as zeros (row N/2 of v_y and w_x, column N/2 of v_x and w_y) carry
energy in the input."""
import ctypes

import numpy as np
import pytest

import coarsen_oracle as co
from backend_util import be, rel_l2  # noqa: F401

B = 3
SIZES = [16, 32]
BOUND = 1e-6
ALPHA = [0, 0.1496590219993, 0.3704009573644, 0.6222557631345, 0.9582821306748, 1]
BETA = [0, -0.4178904745, -1.192151694643, -1.697784692471, -1.514183444257]
GAMMA = [0.1496590219993, 0.3792103129999, 0.8229550293869, 0.6994504559488, 0.1530572479681]


def _indices(N):
    ix = np.concatenate((np.arange(0, N // 2), np.arange(-(N // 2), 0))).astype(np.float64)[:, None]
    iy = np.arange(N // 2 + 1, dtype=np.float64)[None, :]
    return ix, iy


def _as_complex(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def _as_pairs(c):
    return np.stack((c.real, c.imag), axis=-1)


@pytest.mark.parametrize("k0", [1.0, 0.5])      # the domains [0, 2 pi)^2 and [0, 4 pi)^2
@pytest.mark.parametrize("N", SIZES)
def test_kf2d_derivs(be, N, k0):
    rng = np.random.default_rng(10 + N)
    w = rng.standard_normal((B, N, N // 2 + 1, 2)).astype(np.float32)
    hw, out = be.put(w), be.empty((4, B, N, N // 2 + 1, 2))
    assert be.lib.ffno_kf2d_derivs(be.ptr(hw), be.ptr(out), k0, B, N, None) == 0
    got = be.get(out)
    ix, iy = _indices(N)
    kx, ky = k0 * ix, k0 * iy
    k2 = kx ** 2 + ky ** 2
    wc = _as_complex(w)
    psi = wc / np.where(k2 > 0, k2, 1.0)
    psi[:, 0, 0] = 0
    ref = np.stack((1j * ky * psi, -1j * kx * psi, 1j * kx * wc, 1j * ky * wc))
    ref[0][:, :, N // 2] = 0      # v_x, w_y: column N/2;  v_y, w_x: row N/2
    ref[3][:, :, N // 2] = 0
    ref[1][:, N // 2, :] = 0
    ref[2][:, N // 2, :] = 0
    assert np.abs(wc[:, N // 2, :]).min() > 0 and np.abs(wc[:, :, N // 2]).min() > 0      # the input has energy there
    for i, name in enumerate(("v_x", "v_y", "w_x", "w_y")):
        e = rel_l2(got[i], _as_pairs(ref[i]))
        print(f"[kf2d derivs N={N} k0={k0}] {name} {e:.2e}")
        assert e <= BOUND, (name, e)
    for i in (0, 3):
        assert np.all(got[i][:, :, N // 2] == 0.0)
    for i in (1, 2):
        assert np.all(got[i][:, N // 2, :] == 0.0)
    assert np.all(got[:2, :, 0, 0] == 0.0)      # no mean flow: psi_h(0, 0) = 0
    np.testing.assert_array_equal(be.get(hw), w)


def _stage_reference(w, h, adv, N, nu, drag, c, dt, s, kf, f, k0, adv_scale=1.0):
    ix, iy = _indices(N)
    k2 = k0 ** 2 * (ix ** 2 + iy ** 2)
    keep = (9 * (ix ** 2 + iy ** 2) <= N * N).astype(np.float64)
    assert 0 < keep.sum() < keep.size      # the filter keeps at least one bin and drops at least one
    f_h = np.zeros((N, N // 2 + 1), np.complex128)
    f_h[0, kf] = f
    E = -keep * adv_scale * _as_complex(adv) + c * _as_complex(w) + f_h
    h_new = E + (BETA[s] * _as_complex(h) if s else 0.0)
    L = -nu * k2 - drag
    mu = 0.5 * dt * (ALPHA[s + 1] - ALPHA[s])
    return (_as_complex(w) + GAMMA[s] * dt * h_new + mu * L * _as_complex(w)) / (1 - mu * L), h_new, mu


@pytest.mark.parametrize("c", [0.0, -0.1])
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("s", [0, 3])
@pytest.mark.parametrize("N", SIZES)
def test_kf2d_stage(be, N, s, forced, c):
    rng = np.random.default_rng(30 + N + s)
    Nh = N // 2 + 1
    w, h, adv = (rng.standard_normal((B, N, Nh, 2)).astype(np.float32) for _ in range(3))
    nu, drag, dt, k0 = 1e-3, 0.1, 0.5 * (2 * np.pi / N) / 7.0, 1.0
    kf = 4 if forced else 0
    f = -1.0 * kf * (N * N / 2) * np.exp(1j * kf * np.pi / N) if forced else 0.0
    f32 = np.complex64(f)      # the scalars the kernel is handed
    hw, hh, ha = be.put(w), be.put(h if s else np.full_like(h, np.nan)), be.put(adv)      # s = 0 must not read h
    mu = 0.5 * dt * (ALPHA[s + 1] - ALPHA[s])
    rc = be.lib.ffno_kf2d_stage(be.ptr(hw), be.ptr(hh), be.ptr(ha), nu, drag, c, dt, BETA[s], GAMMA[s], mu, kf, float(f32.real),
                                float(f32.imag), k0, 1.0, int(s == 0), B, N, None)
    assert rc == 0
    w_ref, h_ref, _ = _stage_reference(w, h, adv, N, nu, drag, c, dt, s, kf, complex(f32), k0)
    got_w, got_h = be.get(hw), be.get(hh)
    ew, eh = rel_l2(got_w, _as_pairs(w_ref)), rel_l2(got_h, _as_pairs(h_ref))
    print(f"[kf2d stage N={N} s={s} forced={forced} c={c}] w {ew:.2e} h {eh:.2e}")
    assert ew <= BOUND and eh <= BOUND
    if forced:      # the one forced bin, which the whole-array norm would not resolve if it were missed by a rounding
        eb = rel_l2(got_h[:, 0, kf], _as_pairs(h_ref[:, 0, kf]))
        assert abs(f) > 10 * np.abs(_as_complex(adv)).max() and eb <= BOUND, eb
        assert rel_l2(got_w[:, 0, kf], _as_pairs(w_ref[:, 0, kf])) <= BOUND
    np.testing.assert_array_equal(be.get(ha), adv)      # the advection spectrum is only read


def test_kf2d_stage_on_the_doubled_domain(be):
    """k0 = 1/2 (the large_domain files): L uses k0^2 |index|^2, the filter and the forced bin stay in indices.  adv_scale = N^-4
    on an advection spectrum N^4 times too large: what the host passes after unnormalised inverse transforms."""
    N, s, k0, kf = 16, 3, 0.5, 6
    scale = float(N) ** -4
    rng = np.random.default_rng(77)
    w, h, adv = (rng.standard_normal((B, N, N // 2 + 1, 2)).astype(np.float32) for _ in range(3))
    adv *= np.float32(N) ** 4
    nu, drag, c, dt = 0.05, 0.1, -0.1, 0.02
    f = np.complex64(-1.0 * 3.0 * (N * N / 2) * np.exp(1j * kf * np.pi / N))
    hw, hh, ha = be.put(w), be.put(h), be.put(adv)
    mu = 0.5 * dt * (ALPHA[s + 1] - ALPHA[s])
    assert be.lib.ffno_kf2d_stage(be.ptr(hw), be.ptr(hh), be.ptr(ha), nu, drag, c, dt, BETA[s], GAMMA[s], mu, kf, float(f.real),
                                  float(f.imag), k0, scale, 0, B, N, None) == 0
    w_ref, h_ref, _ = _stage_reference(w, h, adv, N, nu, drag, c, dt, s, kf, complex(f), k0, scale)
    assert rel_l2(be.get(hw), _as_pairs(w_ref)) <= BOUND and rel_l2(be.get(hh), _as_pairs(h_ref)) <= BOUND
    other, _, _ = _stage_reference(w, h, adv, N, nu, drag, c, dt, s, kf, complex(f), 1.0, scale)
    assert rel_l2(_as_pairs(other), _as_pairs(w_ref)) > 1e-3      # k0 matters at these values


@pytest.mark.parametrize("N,m", [(16, 8), (16, 4), (32, 8), (64, 32)])
def test_kf2d_downsample(be, N, m):
    """f = 2, 4, 4 and 2; the wrapped halo row (last coarse row) and column (last coarse column) compared on their own.  These
    sizes are one slice per sample (the rule cuts slices of about 1024 coarse cells); the next test has four."""
    rng = np.random.default_rng(50 + N + m)
    vel = rng.standard_normal((2, B, N, N)).astype(np.float32)
    out = be.empty((B, m, m))
    length = 2 * np.pi
    assert be.lib.ffno_kf2d_downsample(be.ptr(be.put(vel)), be.ptr(out), B, N, m, length, None) == 0
    want = co.curl(*co.coarsen_velocity(vel[0], vel[1], m), np.float32(length), np.float32(length))
    got = be.get(out)
    e = rel_l2(got, want)
    print(f"[kf2d downsample N={N} m={m}] {e:.2e}")
    assert e <= BOUND
    assert rel_l2(got[:, -1, :], want[:, -1, :]) <= BOUND and rel_l2(got[:, :, -1], want[:, :, -1]) <= BOUND


def test_kf2d_downsample_several_slices_and_another_length(be):
    """m = 64 from N = 128: 4 slices of 16 coarse rows per sample, the halo row of the last slice wraps to row 0; length 4 pi."""
    N, m, Bs = 128, 64, 2
    rng = np.random.default_rng(5)
    vel = rng.standard_normal((2, Bs, N, N)).astype(np.float32)
    out = be.empty((Bs, m, m))
    assert be.lib.ffno_kf2d_downsample(be.ptr(be.put(vel)), be.ptr(out), Bs, N, m, 4 * np.pi, None) == 0
    want = co.curl(*co.coarsen_velocity(vel[0], vel[1], m), np.float32(4 * np.pi), np.float32(4 * np.pi))
    got = be.get(out)
    assert np.isfinite(got).all() and rel_l2(got, want) <= BOUND
    for i0 in (15, 16, 63):      # the rows at the slice borders and the wrapped one
        assert rel_l2(got[:, i0], want[:, i0]) <= BOUND


def test_kf2d_supported_and_bad_arguments(be):
    lib, p = be.lib, be.ptr
    assert [n for n in range(1, 8200) if lib.ffno_kf2d_supported(n)] == [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    assert lib.ffno_ns2d_supported(1024) == 0      # the other solver's range is untouched
    N = 16
    w, h, out = be.zeros((B, N, N // 2 + 1, 2)), be.zeros((B, N, N // 2 + 1, 2)), be.empty((4, B, N, N // 2 + 1, 2))
    off = lambda t: ctypes.c_void_p(p(t).value + 4)      # noqa: E731   16-byte loads: refused, not read
    assert lib.ffno_kf2d_derivs(p(w), p(out), 1.0, B, 24, None) == -2
    assert lib.ffno_kf2d_derivs(p(w), p(out), 1.0, B, 8, None) == -2
    assert lib.ffno_kf2d_derivs(p(w), p(out), 1.0, B, 8192, None) == -2
    assert lib.ffno_kf2d_derivs(p(w), p(out), 1.0, 1 << 16, 512, None) == -2      # 2^16 x 512 x 257 bins: past the 32-bit index
    assert lib.ffno_kf2d_derivs(None, p(out), 1.0, B, N, None) == -1
    assert lib.ffno_kf2d_derivs(p(w), None, 1.0, B, N, None) == -1
    assert lib.ffno_kf2d_derivs(p(w), p(out), 1.0, 0, N, None) == -1
    assert lib.ffno_kf2d_derivs(p(w), p(out), 0.0, B, N, None) == -1
    assert lib.ffno_kf2d_derivs(off(w), p(out), 1.0, B, N, None) == -1

    adv = be.zeros((B, N, N // 2 + 1, 2))

    def stage(w_=p(w), h_=p(h), a_=p(adv), kf=4, n=N, b=B, fr=1.0, k0=1.0, sc=1.0):
        return lib.ffno_kf2d_stage(w_, h_, a_, 1e-3, 0.1, 0.0, 1e-2, 0.0, 0.1, 1e-3, kf, fr, 0.0, k0, sc, 1, b, n, None)

    assert stage() == 0
    assert stage(w_=None) == -1 and stage(h_=None) == -1 and stage(a_=None) == -1 and stage(b=0) == -1
    assert stage(w_=off(w)) == -1 and stage(h_=off(h)) == -1 and stage(a_=off(adv)) == -1
    assert stage(n=24) == -2 and stage(n=8) == -2
    assert stage(k0=0.0) == -1 and stage(k0=float('nan')) == -1 and stage(sc=0.0) == -1 and stage(sc=-1.0) == -1
    assert stage(kf=N // 2) == -1 and stage(kf=-1) == -1 and stage(kf=N // 2 - 1) == 0
    assert stage(kf=0) == -1 and stage(kf=0, fr=0.0) == 0      # kf = 0 is "no forcing" and takes no amplitude

    vel, o = be.zeros((2, B, N, N)), be.empty((B, 8, 8))
    assert lib.ffno_kf2d_downsample(p(vel), p(o), B, N, 8, 6.28, None) == 0
    assert lib.ffno_kf2d_downsample(None, p(o), B, N, 8, 6.28, None) == -1
    assert lib.ffno_kf2d_downsample(p(vel), None, B, N, 8, 6.28, None) == -1
    assert lib.ffno_kf2d_downsample(p(vel), p(o), B, N, 6, 6.28, None) == -1      # 6 does not divide 16
    assert lib.ffno_kf2d_downsample(p(vel), p(o), B, N, 8, 0.0, None) == -1
    assert lib.ffno_kf2d_downsample(p(vel), p(o), B, 24, 8, 6.28, None) == -2


@pytest.mark.gpu
def test_kf2d_largest_grid_on_the_gpu():
    """N = 4096, B = 1: 4.2 M pairs of bins against 8192 x 256 threads, so the grid-stride loops of derivs and stage take a second
    and a third trip (no smaller supported shape does: 2048 x 2048 is 1.05 M pairs), and the index arithmetic runs at its largest
    values (k2 up to 2^23).  Then the reduction 2048 -> 1024: 1024 slices of one coarse row each.  Too slow for the emulator."""
    from backend_util import Backend
    be = Backend("gpu")
    N, Bs, s, k0 = 4096, 1, 3, 1.0
    Nh = N // 2 + 1
    assert Bs * N * Nh // 2 > 2 * 8192 * 256
    rng = np.random.default_rng(4096)
    w, h, adv = (rng.standard_normal((Bs, N, Nh, 2), dtype=np.float32) for _ in range(3))
    hw, out = be.put(w), be.empty((4, Bs, N, Nh, 2))
    assert be.lib.ffno_kf2d_derivs(be.ptr(hw), be.ptr(out), k0, Bs, N, None) == 0
    got = be.get(out)
    ix, iy = _indices(N)
    k2 = ix ** 2 + iy ** 2
    wc = _as_complex(w)
    psi = wc / np.where(k2 > 0, k2, 1.0)
    sx, sy = ix.copy(), iy.copy()
    sx[N // 2, 0], sy[0, N // 2] = 0.0, 0.0
    for i, (name, ref) in enumerate((("v_x", 1j * sy * psi), ("v_y", -1j * sx * psi), ("w_x", 1j * sx * wc), ("w_y", 1j * sy * wc))):
        e = rel_l2(got[i], _as_pairs(ref))
        print(f"[kf2d derivs N={N}] {name} {e:.2e}")
        assert e <= BOUND, (name, e)
    del got, psi, out
    nu, drag, c, dt, kf = 1e-3, 0.1, -0.1, 0.5 * (2 * np.pi / N) / 7.0, 4
    f = np.complex64(-1.0 * kf * (N * N / 2) * np.exp(1j * kf * np.pi / N))
    hh, ha = be.put(h), be.put(adv)
    mu = 0.5 * dt * (ALPHA[s + 1] - ALPHA[s])
    assert be.lib.ffno_kf2d_stage(be.ptr(hw), be.ptr(hh), be.ptr(ha), nu, drag, c, dt, BETA[s], GAMMA[s], mu, kf, float(f.real),
                                  float(f.imag), k0, 1.0, 0, Bs, N, None) == 0
    w_ref, h_ref, _ = _stage_reference(w, h, adv, N, nu, drag, c, dt, s, kf, complex(f), k0)
    ew, eh = rel_l2(be.get(hw), _as_pairs(w_ref)), rel_l2(be.get(hh), _as_pairs(h_ref))
    print(f"[kf2d stage N={N}] w {ew:.2e} h {eh:.2e}")
    assert ew <= BOUND and eh <= BOUND
    assert rel_l2(be.get(hh)[:, 0, kf], _as_pairs(h_ref[:, 0, kf])) <= BOUND
    N, m = 2048, 1024
    vel = rng.standard_normal((2, Bs, N, N), dtype=np.float32)
    o = be.empty((Bs, m, m))
    assert be.lib.ffno_kf2d_downsample(be.ptr(be.put(vel)), be.ptr(o), Bs, N, m, 2 * np.pi, None) == 0
    want = co.curl(*co.coarsen_velocity(vel[0], vel[1], m), np.float32(2 * np.pi), np.float32(2 * np.pi))
    e = rel_l2(be.get(o), want)
    print(f"[kf2d downsample N={N} m={m}] {e:.2e}")
    assert e <= BOUND
