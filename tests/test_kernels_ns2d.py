"""The three streaming kernels of the Navier-Stokes solver step (csrc/ffno_ns2d.h: ffno_ns2d_derivs, ffno_ns2d_advect,
ffno_ns2d_cn_update) and ffno_ns2d_supported through the C ABI against float64 numpy, on the emulator and on an MI355X.
Every output is a handful of fp32 roundings of its float64 value: relative L2 <= 1e-6.  The input of derivs is a random spectrum
WITHOUT Hermitian symmetry, so the bins the kernel has to write as zeros (row N/2 of v and w_x, column N/2 of q and w_y) carry
energy in the input."""
import numpy as np
import pytest

from backend_util import be, rel_l2  # noqa: F401

B = 3
SIZES = [8, 16]      # 8: the smallest supported grid (5 columns); 16: 9 columns, more than one row per 16-byte pair pattern
BOUND = 1e-6


def _wavenumbers(N):
    kx = np.concatenate((np.arange(0, N // 2), np.arange(-(N // 2), 0))).astype(np.float64)[:, None]
    ky = np.arange(N // 2 + 1, dtype=np.float64)[None, :]
    lap = 4 * np.pi ** 2 * (kx ** 2 + ky ** 2)
    lap[0, 0] = 1.0
    return kx, ky, lap


def _as_complex(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def _as_pairs(c):
    return np.stack((c.real, c.imag), axis=-1)


@pytest.mark.parametrize("N", SIZES)
def test_ns2d_derivs(be, N):
    rng = np.random.default_rng(10 + N)
    w = rng.standard_normal((B, N, N // 2 + 1, 2)).astype(np.float32)
    hw, out = be.put(w), be.empty((4, B, N, N // 2 + 1, 2))
    assert be.lib.ffno_ns2d_derivs(be.ptr(hw), be.ptr(out), B, N, None) == 0
    got = be.get(out)
    kx, ky, lap = _wavenumbers(N)
    wc = _as_complex(w)
    ref = np.stack((2j * np.pi * ky * wc / lap, -2j * np.pi * kx * wc / lap, 2j * np.pi * kx * wc, 2j * np.pi * ky * wc))
    ref[0][:, :, N // 2] = 0      # q, w_y: column N/2;  v, w_x: row N/2
    ref[3][:, :, N // 2] = 0
    ref[1][:, N // 2, :] = 0
    ref[2][:, N // 2, :] = 0
    assert np.abs(wc[:, N // 2, :]).min() > 0 and np.abs(wc[:, :, N // 2]).min() > 0      # the input has energy there
    for i, name in enumerate(("q", "v", "w_x", "w_y")):
        e = rel_l2(got[i], _as_pairs(ref[i]))
        print(f"[ns2d derivs N={N}] {name} {e:.2e}")
        assert e <= BOUND, (name, e)
    for i in (0, 3):
        assert np.all(got[i][:, :, N // 2] == 0.0)
    for i in (1, 2):
        assert np.all(got[i][:, N // 2, :] == 0.0)
    np.testing.assert_array_equal(be.get(hw), w)


@pytest.mark.parametrize("N", SIZES)
def test_ns2d_advect(be, N):
    rng = np.random.default_rng(20 + N)
    f = rng.standard_normal((4, B, N, N)).astype(np.float32)
    hf, out = be.put(f), be.empty((B, N, N))
    assert be.lib.ffno_ns2d_advect(be.ptr(hf), be.ptr(out), B * N * N, None) == 0
    f64 = f.astype(np.float64)
    e = rel_l2(be.get(out), f64[0] * f64[2] + f64[1] * f64[3])
    print(f"[ns2d advect N={N}] {e:.2e}")
    assert e <= BOUND


@pytest.mark.parametrize("force", ["none", "shared", "batched"])
@pytest.mark.parametrize("N", SIZES)
def test_ns2d_cn_update(be, N, force):
    rng = np.random.default_rng(30 + N)
    Nh = N // 2 + 1
    w = rng.standard_normal((B, N, Nh, 2)).astype(np.float32)
    F = rng.standard_normal((B, N, Nh, 2)).astype(np.float32)
    fh = {"none": None, "shared": rng.standard_normal((N, Nh, 2)), "batched": rng.standard_normal((B, N, Nh, 2))}[force]
    fh = None if fh is None else fh.astype(np.float32)
    visc = np.array([1e-3, 3e-2, 2e-4], np.float32)
    dt = np.float32(1e-2)
    hw, hF, hf, hv = be.put(w), be.put(F), be.put(fh), be.put(visc)
    assert be.lib.ffno_ns2d_cn_update(be.ptr(hw), be.ptr(hF), be.ptr(hf), be.ptr(hv), float(dt), int(force == "batched"), B, N,
                                      None) == 0
    kx, ky, lap = _wavenumbers(N)
    keep = ((np.abs(kx) <= (2.0 / 3.0) * (N // 2)) & (np.abs(ky) <= (2.0 / 3.0) * (N // 2))).astype(np.float64)
    assert 0 < keep.sum() < keep.size
    factor = 0.5 * float(dt) * visc.astype(np.float64)[:, None, None] * lap
    fc = 0.0 if fh is None else _as_complex(fh)
    ref = (-float(dt) * _as_complex(F) * keep + float(dt) * fc + (1 - factor) * _as_complex(w)) / (1 + factor)
    e = rel_l2(be.get(hw), _as_pairs(ref))
    print(f"[ns2d cn_update N={N} force={force}] {e:.2e}")
    assert e <= BOUND
    np.testing.assert_array_equal(be.get(hF), F)      # F_h is only read


def test_ns2d_supported_and_bad_arguments(be):
    lib, p = be.lib, be.ptr
    assert [n for n in range(1, 1100) if lib.ffno_ns2d_supported(n)] == [8, 16, 32, 64, 128, 256, 512]
    N = 8
    w, out = be.zeros((B, N, N // 2 + 1, 2)), be.empty((4, B, N, N // 2 + 1, 2))
    visc = be.put(np.full(B, 1e-3, np.float32))
    assert lib.ffno_ns2d_derivs(p(w), p(out), B, 12, None) == -2
    assert lib.ffno_ns2d_derivs(p(w), p(out), B, 4, None) == -2
    assert lib.ffno_ns2d_derivs(None, p(out), B, N, None) == -1
    assert lib.ffno_ns2d_derivs(p(w), p(out), 0, N, None) == -1
    assert lib.ffno_ns2d_advect(p(out), p(w), 6, None) == -1           # not a multiple of 4
    assert lib.ffno_ns2d_advect(p(out), None, 8, None) == -1
    assert lib.ffno_ns2d_cn_update(p(w), p(w), None, None, 1e-2, 0, B, N, None) == -1
    assert lib.ffno_ns2d_cn_update(p(w), p(w), None, p(visc), 1e-2, 0, B, 24, None) == -2
    # 16-byte loads: a pointer that is not 16-byte aligned is refused, not read
    import ctypes
    assert lib.ffno_ns2d_derivs(ctypes.c_void_p(p(w).value + 4), p(out), B, N, None) == -1
