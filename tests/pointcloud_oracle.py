"""Float64 restatement of the point-cloud F-FNO's non-uniform DFT (reference
fourierflow/modules/factorized_fno/point_cloud_2d.py, SpectralConv2d.fft2d :95-131 and .ifft2d :133-159, with the corner
slicing / concatenation of :54-67), written literally so torch autograd supplies independent gradients; plus the closed form
of ifft2d's `flip(-1, -2).conj()` completion that the kernels implement."""
import numpy as np
import torch


def _wavenumbers(modes1, modes2):
    m1, m2 = 2 * modes1, 2 * modes2 - 1
    k_x1 = torch.cat((torch.arange(0, modes1), torch.arange(-modes1, 0)), 0).reshape(m1, 1).repeat(1, m2)
    k_x2 = torch.cat((torch.arange(0, modes2), torch.arange(-(modes2 - 1), 0)), 0).reshape(1, m2).repeat(m1, 1)
    return k_x1.double(), k_x2.double()


def _basis(xi, modes1, modes2, sign):
    B, N = xi.shape[:2]
    k_x1, k_x2 = _wavenumbers(modes1, modes2)
    m1, m2 = k_x1.shape
    K1 = torch.outer(xi[..., 0].reshape(-1), k_x1.reshape(-1)).reshape(B, N, m1, m2)
    K2 = torch.outer(xi[..., 1].reshape(-1), k_x2.reshape(-1)).reshape(B, N, m1, m2)
    return torch.exp(sign * 1j * 2 * np.pi * (K1 + K2))


def fft2d(u, xi, modes1, modes2):
    """u [B, C, N], xi [B, N, 2] (float64) -> complex128 [B, C, 2 modes1, modes2]: fft2d + cat of its two corners."""
    Y = torch.einsum("bcn,bnxy->bcxy", u + 0j, _basis(xi, modes1, modes2, -1))
    return torch.cat([Y[:, :, :modes1, :modes2], Y[:, :, -modes1:, :modes2]], dim=-2)


def ifft2d(spec, xi):
    """complex128 spec [B, C, 2 m1, m2], xi [B, N, 2] -> [B, C, N], the reference's literal completion."""
    modes1, modes2 = spec.shape[2] // 2, spec.shape[3]
    u_ft2 = spec[..., 1:].flip(-1, -2).conj()
    u_ft = torch.cat([spec, u_ft2], dim=-1)
    return torch.einsum("bcxy,bnxy->bcn", u_ft, _basis(xi, modes1, modes2, 1)).real


def ifft2d_closed(spec, xi):
    """The same map as ifft2d:  Re sum_{r,j} V E (1 + [j >= 1] exp(2 pi i xi_1)) over the kept modes only."""
    modes1, modes2 = spec.shape[2] // 2, spec.shape[3]
    k1 = torch.cat((torch.arange(0, modes1), torch.arange(-modes1, 0))).double()
    k2 = torch.arange(0, modes2).double()
    th = xi[..., 0, None, None] * k1[:, None] + xi[..., 1, None, None] * k2[None, :]
    E = torch.exp(2j * np.pi * th)
    q = 1 + (k2 >= 1).double() * torch.exp(2j * np.pi * xi[..., 0])[..., None, None]
    return torch.einsum("bcxy,bnxy->bcn", spec, E * q).real
