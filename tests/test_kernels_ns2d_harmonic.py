"""The two kernels of the time-varying random force (csrc/ffno_ns2d.h: ffno_ns2d_cn_update_harmonic, ffno_ns2d_harmonic_force)
through the C ABI against float64 numpy, on the emulator and on an MI355X.  The float64 side goes the plain way: the force field
is evaluated on the grid, transformed with fft2 and cut to the half spectrum; it knows nothing of the 4 x cycles bins the kernel
computes.  Every output is a handful of fp32 roundings of its float64 value: relative L2 <= 1e-6 (the bound of
test_kernels_ns2d.py).  N = 8 with cycles = 3 is the largest count allowed there, and with 5 columns the 16-byte pairs straddle
rows, so the column-0 force bins arrive as the second bin of a pair as well as the first."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ns2d_oracle as oracle
from backend_util import Backend, be, rel_l2  # noqa: F401

B = 3
CASES = [(8, 3), (16, 1), (16, 2)]      # (N, cycles)
BOUND = 1e-6
PHI, SCALING, DT = 1.8, 0.1, 1e-2


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


def _field(amp, N, scaling, phi):
    """amp [b, cycles, 6] -> the force [b, N, N] at phase phi, in float64."""
    a = amp.astype(np.float64)
    g = np.arange(N, dtype=np.float64) / N
    X, Y = g[:, None], g[None, :]
    f = np.zeros((a.shape[0], N, N))
    for p in range(1, a.shape[1] + 1):
        k = 2 * np.pi * p
        for i, term in enumerate((np.sin(k * X + phi) + 0 * Y, np.cos(k * X + phi) + 0 * Y, np.sin(k * Y + phi) + 0 * X,
                                  np.cos(k * Y + phi) + 0 * X, np.sin(k * (X + Y) + phi), np.cos(k * (X + Y) + phi))):
            f += a[:, p - 1, i][:, None, None] * term
    return scaling * f


def _update(w, F, fc, visc, dt, N):
    kx, ky, lap = _wavenumbers(N)
    keep = ((np.abs(kx) <= (2.0 / 3.0) * (N // 2)) & (np.abs(ky) <= (2.0 / 3.0) * (N // 2))).astype(np.float64)
    factor = 0.5 * dt * visc.astype(np.float64)[:, None, None] * lap
    return (-dt * _as_complex(F) * keep + dt * fc + (1 - factor) * _as_complex(w)) / (1 + factor)


def _operands(rng, b, N, cycles):
    Nh = N // 2 + 1
    w = rng.standard_normal((b, N, Nh, 2), dtype=np.float32)
    F = rng.standard_normal((b, N, Nh, 2), dtype=np.float32)
    amp = rng.random((b, cycles, 6), dtype=np.float32)
    visc = rng.uniform(2e-4, 3e-2, b).astype(np.float32)
    return w, F, amp, visc


def _harmonic_update(be, w, F, amp, visc, N, cycles, phi):
    hw, hF, ha, hv = be.put(w), be.put(F), be.put(amp), be.put(visc)
    rc = be.lib.ffno_ns2d_cn_update_harmonic(be.ptr(hw), be.ptr(hF), be.ptr(ha), be.ptr(hv), DT, SCALING, math.cos(phi), math.sin(phi),
                                             cycles, len(w), N, None)
    assert rc == 0
    return be.get(hw), be.get(hF), be.get(ha)


@pytest.mark.parametrize("N,cycles", CASES)
def test_ns2d_cn_update_harmonic(be, N, cycles):
    w, F, amp, visc = _operands(np.random.default_rng(40 + N + cycles), B, N, cycles)
    got, F_after, amp_after = _harmonic_update(be, w, F, amp, visc, N, cycles, PHI)
    f_h = np.fft.fft2(_field(amp, N, SCALING, PHI))[:, :, :N // 2 + 1]
    e = rel_l2(got, _as_pairs(_update(w, F, f_h, visc, DT, N)))
    print(f"[ns2d cn_update_harmonic N={N} cycles={cycles}] {e:.2e}")
    assert e <= BOUND
    np.testing.assert_array_equal(F_after, F)
    np.testing.assert_array_equal(amp_after, amp)
    # against the forceless update of the same inputs: exactly 4 cycles bins per sample differ
    hw, hF, hv = be.put(w), be.put(F), be.put(visc)
    assert be.lib.ffno_ns2d_cn_update(be.ptr(hw), be.ptr(hF), None, be.ptr(hv), DT, 0, B, N, None) == 0
    differ = (got != be.get(hw)).any(axis=-1).reshape(B, -1).sum(axis=1)
    assert list(differ) == [4 * cycles] * B, differ


@pytest.mark.parametrize("N,cycles", CASES)
@pytest.mark.parametrize("phi", [0.0, PHI, 1234.5])
def test_ns2d_harmonic_force(be, N, cycles, phi):
    amp = np.random.default_rng(50 + N + cycles).random((B, cycles, 6), dtype=np.float32)
    ha, hf = be.put(amp), be.empty((B, N, N))
    assert be.lib.ffno_ns2d_harmonic_force(be.ptr(ha), be.ptr(hf), SCALING, math.cos(phi), math.sin(phi), cycles, B, N, None) == 0
    got = be.get(hf)
    e = rel_l2(got, _field(amp, N, SCALING, phi))
    print(f"[ns2d harmonic_force N={N} cycles={cycles} phi={phi}] {e:.2e}")
    assert e <= BOUND
    np.testing.assert_array_equal(be.get(ha), amp)
    if phi == 0.0:
        ref = oracle.force_field("random", B, N, torch.float64, amp.transpose(1, 2, 0), cycles, SCALING).numpy()
        assert rel_l2(got, ref) <= BOUND


def test_ns2d_harmonic_bad_arguments(be):
    lib = be.lib
    N, cycles = 8, 2

    def p(h):      # a handle of the backend, or a raw pointer as it is
        return h if isinstance(h, ctypes.c_void_p) else be.ptr(h)

    w, F = be.zeros((B, N, N // 2 + 1, 2)), be.zeros((B, N, N // 2 + 1, 2))
    amp, visc, f = be.zeros((B, cycles, 6)), be.put(np.full(B, 1e-3, np.float32)), be.zeros((B, N, N))

    def update(w_=w, F_=F, amp_=amp, visc_=visc, cycles_=cycles, B_=B, N_=N):
        return lib.ffno_ns2d_cn_update_harmonic(p(w_), p(F_), p(amp_), p(visc_), 1e-2, 0.1, 1.0, 0.0, cycles_, B_, N_, None)

    def force(amp_=amp, f_=f, cycles_=cycles, B_=B, N_=N):
        return lib.ffno_ns2d_harmonic_force(p(amp_), p(f_), 0.1, 1.0, 0.0, cycles_, B_, N_, None)

    assert update() == 0 and force() == 0
    for call in (update, force):
        assert call(cycles_=0) == -2
        assert call(cycles_=N // 2) == -2      # rows p and N - p coincide at p = N/2
        assert call(N_=12) == -2
        assert call(N_=4) == -2
        assert call(amp_=None) == -1
        assert call(B_=0) == -1
    assert update(F_=None) == -1 and update(visc_=None) == -1 and force(f_=None) == -1
    # 16-byte accesses: a pointer that is not 16-byte aligned is refused, not read
    assert update(w_=ctypes.c_void_p(p(w).value + 4)) == -1
    assert force(f_=ctypes.c_void_p(p(f).value + 4)) == -1


@pytest.mark.gpu
def test_ns2d_harmonic_where_the_grid_stride_loop_turns_over():
    """N = 512, B = 33: 2 171 136 bin pairs, more than one sweep of 8192 x 256 threads; the force field has 2 162 688 float4."""
    be = Backend("gpu")
    N, b, cycles = 512, 33, 2
    w, F, amp, visc = _operands(np.random.default_rng(60), b, N, cycles)
    assert w.size // 4 > 8192 * 256 and b * N * N // 4 > 8192 * 256
    got, F_after, _ = _harmonic_update(be, w, F, amp, visc, N, cycles, PHI)
    field = _field(amp, N, SCALING, PHI)
    e = rel_l2(got, _as_pairs(_update(w, F, np.fft.fft2(field)[:, :, :N // 2 + 1], visc, DT, N)))
    hf = be.empty((b, N, N))
    assert be.lib.ffno_ns2d_harmonic_force(be.ptr(be.put(amp)), be.ptr(hf), SCALING, math.cos(PHI), math.sin(PHI), cycles, b, N, None) == 0
    ef = rel_l2(be.get(hf), field)
    print(f"[ns2d harmonic N=512 B=33] update {e:.2e}, force {ef:.2e}")
    assert e <= BOUND and ef <= BOUND
    np.testing.assert_array_equal(F_after, F)
