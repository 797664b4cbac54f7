"""Restatement of the 2-D Navier-Stokes generator for the tests, written from the formulas in float64 or float32 torch:

    vorticity equation   w_t + u . grad(w) = nu lap(w) + f     on the periodic unit square, u = (psi_y, -psi_x), -lap(psi) = w
    pseudo-spectral:     derivatives as i 2 pi k in Fourier space, the product u . grad(w) on the grid, 2/3-rule dealiasing
    Crank-Nicolson:      w_h' = (-dt F_h + dt f_h + (1 - a) w_h) / (1 + a),   a = dt nu L / 2,   L = 4 pi^2 |k|^2  (L[0, 0] = 1)

in the FULL complex form: every transform is an N x N complex FFT and the physical fields are the real parts of the inverse
transforms.  (That is the form whose Nyquist behaviour the half-spectrum kernels of csrc/ffno_ns2d.h reproduce by writing zeros:
the real part of the inverse transform drops i k w_h wherever k is an axis' Nyquist wavenumber.)  Also the Gaussian random field
of the initial vorticity and the four force fields.
"""
import math

import numpy as np
import torch


def wavenumbers(N, dtype, device=None):
    k = torch.cat((torch.arange(0, N // 2, device=device), torch.arange(-(N // 2), 0, device=device))).to(dtype)
    return k[:, None].expand(N, N), k[None, :].expand(N, N)      # k_x varies along axis 0, k_y along axis 1


def tables(N, dtype, device=None):
    """(k_x, k_y, L, dealiasing mask), each [N, N]: what a solver computes once per run."""
    kx, ky = wavenumbers(N, dtype, device)
    lap = 4 * math.pi ** 2 * (kx ** 2 + ky ** 2)
    lap[0, 0] = 1.0
    mask = ((kx.abs() <= (2.0 / 3.0) * (N // 2)) & (ky.abs() <= (2.0 / 3.0) * (N // 2))).to(dtype)
    return kx, ky, lap, mask


def force_field(kind, B, N, dtype, amplitudes=None, cycles=None, scaling=None):
    """li / kolmogorov: [N, N]; random: [B, N, N] from amplitudes [cycles, 6, B] (sin kx, cos kx, sin ky, cos ky, sin k(x+y),
    cos k(x+y) per cycle); none: None."""
    if kind == "none":
        return None
    g = torch.arange(N, dtype=dtype) / N
    X, Y = g[:, None].expand(N, N), g[None, :].expand(N, N)
    if kind == "li":
        return 0.1 * (torch.sin(2 * math.pi * (X + Y)) + torch.cos(2 * math.pi * (X + Y)))
    if kind == "kolmogorov":
        return -4 * torch.cos(4 * (2 * math.pi * Y))
    assert kind == "random"
    a = torch.as_tensor(amplitudes, dtype=dtype)
    f = torch.zeros(B, N, N, dtype=dtype)
    for p in range(1, cycles + 1):
        k = 2 * math.pi * p
        terms = (torch.sin(k * X), torch.cos(k * X), torch.sin(k * Y), torch.cos(k * Y), torch.sin(k * (X + Y)), torch.cos(k * (X + Y)))
        for i, term in enumerate(terms):
            f = f + a[p - 1, i][:, None, None] * term
    return f * scaling


def step(w_h, f_h, nu, dt, tabs):
    """One Crank-Nicolson step of the full complex spectrum w_h [B, N, N]; nu [B]; tabs = tables(N, ...)."""
    kx, ky, lap, mask = tabs
    psi_h = w_h / lap

    def grid(spec):
        return torch.fft.ifft2(spec).real

    u = grid(2j * math.pi * ky * psi_h)
    v = grid(-2j * math.pi * kx * psi_h)
    w_x = grid(2j * math.pi * kx * w_h)
    w_y = grid(2j * math.pi * ky * w_h)
    F_h = torch.fft.fft2(u * w_x + v * w_y) * mask
    a = 0.5 * dt * nu[:, None, None] * lap
    return (-dt * F_h + dt * f_h + (1 - a) * w_h) / (1 + a)


def solve(w0, nu, n_steps, dt, record_every, f=None, dtype=torch.float64):
    """w0 [B, N, N] (numpy), nu scalar or [B], f None / [N, N] / [B, N, N] -> snapshots [B, N, N, n_steps // record_every]
    (numpy, of ``dtype``)."""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    w0 = torch.as_tensor(np.asarray(w0), dtype=dtype)
    B = w0.shape[0]
    nu = torch.as_tensor(np.broadcast_to(np.asarray(nu, np.float64), (B,)).copy(), dtype=dtype)
    f_h = torch.zeros((), dtype=cdt) if f is None else torch.fft.fft2(torch.as_tensor(np.asarray(f), dtype=dtype))
    w_h = torch.fft.fft2(w0)
    tabs = tables(w0.shape[-1], dtype)
    out = []
    for j in range(n_steps):
        w_h = step(w_h, f_h, nu, dt, tabs)
        if (j + 1) % record_every == 0:
            out.append(torch.fft.ifft2(w_h).real)
    return torch.stack(out, dim=-1).numpy()


def gaussian_rf(noise, alpha, tau, sigma=None):
    """The field GaussianRF(2, size, alpha, tau, sigma).sample draws from noise [n, size, size, 2] ~ N(0, 1): the inverse transform
    of noise scaled by size^2 sqrt(2) sigma (4 pi^2 |k|^2 + tau^2)^(-alpha / 2), without the mean mode; sigma defaults to
    tau^(alpha - 1)."""
    noise = torch.as_tensor(np.asarray(noise), dtype=torch.float64)
    size = noise.shape[1]
    if sigma is None:
        sigma = tau ** (0.5 * (2 * alpha - 2))
    kx, ky = wavenumbers(size, torch.float64)
    amp = size ** 2 * math.sqrt(2.0) * sigma * (4 * math.pi ** 2 * (kx ** 2 + ky ** 2) + tau ** 2) ** (-alpha / 2.0)
    amp[0, 0] = 0.0
    return torch.fft.ifft2(amp * torch.view_as_complex(noise.contiguous())).real.numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
