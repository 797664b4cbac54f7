"""Non-uniform DFT of the point-cloud F-FNO (ops.point_fft2d / ops.point_ifft2d over ffno_nudft_*) against the float64
restatement of the reference's SpectralConv2d.fft2d / .ifft2d in tests/pointcloud_oracle.py: forward results <= 1e-5,
gradients (du, dV, dxi) <= 5e-5 rel-L2, on the emulator and on an MI355X.

Worst measured figures at the edge cases (the second CASES line: modes1 / modes2 = 1, one channel, 972 points):
    spec / out                        emulator 5.7e-7, MI355X 5.7e-7 (fft2d at (16, 16, 9, 972): 972 terms per mode)
    du, dV, dxi                       emulator 5.6e-7, MI355X 5.6e-7 (dV at (16, 16, 9, 972))
    at the four cases with modes1 or modes2 below 5 or C = 1: results <= 1.7e-7, gradients <= 1.6e-7 on both"""
import numpy as np
import pytest
import torch

import pointcloud_oracle as po
from backend_util import Backend, BACKENDS, host_device, rel_l2  # noqa: F401  (host_device is a fixture)

# (modes1, modes2, channels, points): modes 12 / 16, the W = 32 / 64 widths of the elasticity configs and the 3 channels [x, y, 1]
# of fc0's affine input; 100, 130 and 70 points are not multiples of the 64-point tile; modes1 != modes2 both ways (16 x 9: 288
# modes per channel, a partial second 256-mode tile)
CASES = [(12, 12, 32, 100), (16, 16, 64, 130), (16, 16, 3, 100), (12, 12, 3, 37), (16, 9, 32, 100), (5, 16, 3, 70)]
# the smallest mode counts ffno_nudft_supported admits: modes1 = 1 (the k1 twiddle table has three rows, -1, 0 and the shifted
# +1), modes2 = 1 (only the column j = 0, which takes no shifted row), both at once, one channel (seven of the eight staged
# channel slots empty) on exactly one 64-point tile; and 972 points = 15 tiles of 64 and one of 12, the shipped point count
CASES += [(1, 1, 3, 70), (1, 16, 9, 70), (16, 1, 9, 70), (2, 2, 1, 64), (16, 16, 9, 972)]


def _inputs(C, N, seed, B=2, lo=-0.45, hi=1.6):
    """xi on [lo, hi]^2: the deformed coordinates leave the unit square.  Every input is an fp32 value, so the float64 oracle
    sees exactly what the kernels see."""
    rng = np.random.default_rng(seed)
    xi = rng.uniform(lo, hi, (B, N, 2)).astype(np.float32).astype(np.float64)
    u = rng.standard_normal((B, C, N)).astype(np.float32).astype(np.float64)
    return u, xi


def _spec(B, C, m1, seed, m2=None):
    m2 = m1 if m2 is None else m2
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, C, 2 * m1, m2)) + 1j * rng.standard_normal((B, C, 2 * m1, m2))).astype(np.complex64).astype(
        np.complex128)


def _dev(a, device, grad=True, dtype=torch.float32):
    return torch.tensor(a, dtype=dtype, device=device).requires_grad_(grad)


def test_closed_form_of_the_flip_conj_completion():
    """A check of tests/pointcloud_oracle.py, not of the kernels: its closed form (what the kernels compute) is the reference's
    literal `flip(-1, -2).conj()` formula, and it is NOT the textbook Hermitian completion 2 Re - DC.  The operator tests below
    compare the kernels with the literal formula."""
    u, xi = _inputs(4, 50, 1)
    V = torch.tensor(_spec(2, 4, 6, 2))
    xt = torch.tensor(xi)
    lit = po.ifft2d(V, xt)
    assert rel_l2(po.ifft2d_closed(V, xt), lit) < 1e-12
    k1 = torch.cat((torch.arange(0, 6), torch.arange(-6, 0))).double()
    E = torch.exp(2j * np.pi * (xt[..., 0, None, None] * k1[:, None] + xt[..., 1, None, None] * torch.arange(6).double()))
    herm = torch.einsum("bcxy,bnxy->bcn", V, E * (1 + (torch.arange(6) >= 1).double())).real
    assert rel_l2(herm, lit) > 0.1


@pytest.mark.parametrize("m1,m2,C,N", CASES)
def test_point_fft2d_and_adjoint(host_device, m1, m2, C, N):
    from fourierflow_amd import ops
    u, xi = _inputs(C, N, 10 + m1 + m2 + C)
    ut, xt = _dev(u, host_device), _dev(xi, host_device)
    spec = ops.point_fft2d(ut, xt, m1, m2)
    assert spec.dtype == torch.complex64 and spec.shape == (2, C, 2 * m1, m2)
    u64, x64 = torch.tensor(u, requires_grad=True), torch.tensor(xi, requires_grad=True)
    ref = po.fft2d(u64, x64, m1, m2)
    e_fwd = rel_l2(torch.view_as_real(spec).detach().cpu().numpy(), torch.view_as_real(ref).detach().numpy())
    G = _spec(2, C, m1, 99, m2)
    du, dxi = torch.autograd.grad(spec, (ut, xt), torch.tensor(G, dtype=torch.complex64, device=host_device))
    rdu, rdxi = torch.autograd.grad(ref, (u64, x64), torch.tensor(G))
    e_du, e_dxi = rel_l2(du.cpu().numpy(), rdu.numpy()), rel_l2(dxi.cpu().numpy(), rdxi.numpy())
    print(f"[nudft fft2d m1={m1} m2={m2} C={C} N={N}] spec {e_fwd:.2e}, du {e_du:.2e}, dxi {e_dxi:.2e}")
    assert e_fwd < 1e-5
    assert e_du < 5e-5
    assert e_dxi < 5e-5


@pytest.mark.parametrize("m1,m2,C,N", CASES)
def test_point_ifft2d_and_adjoint(host_device, m1, m2, C, N):
    from fourierflow_amd import ops
    _, xi = _inputs(C, N, 20 + m1 + m2 + C)
    V = _spec(2, C, m1, 30 + m1 + m2, m2)
    Vt = torch.tensor(V, dtype=torch.complex64, device=host_device).requires_grad_(True)
    xt = _dev(xi, host_device)
    out = ops.point_ifft2d(Vt, xt)
    assert out.dtype == torch.float32 and out.shape == (2, C, N)
    V64, x64 = torch.tensor(V, requires_grad=True), torch.tensor(xi, requires_grad=True)
    ref = po.ifft2d(V64, x64)
    e_fwd = rel_l2(out.detach().cpu().numpy(), ref.detach().numpy())
    g = np.random.default_rng(7).standard_normal((2, C, N)).astype(np.float32).astype(np.float64)
    dV, dxi = torch.autograd.grad(out, (Vt, xt), torch.tensor(g, dtype=torch.float32, device=host_device))
    rdV, rdxi = torch.autograd.grad(ref, (V64, x64), torch.tensor(g))
    e_dV = rel_l2(torch.view_as_real(dV).cpu().numpy(), torch.view_as_real(rdV).numpy())
    e_dxi = rel_l2(dxi.cpu().numpy(), rdxi.numpy())
    print(f"[nudft ifft2d m1={m1} m2={m2} C={C} N={N}] out {e_fwd:.2e}, dV {e_dV:.2e}, dxi {e_dxi:.2e}")
    assert e_fwd < 1e-5
    assert e_dV < 5e-5
    assert e_dxi < 5e-5


def test_far_coordinates_keep_their_phase(host_device):
    """xi up to |16|: k xi is reduced modulo 1 exactly, so the phase stays accurate where a plain fp32 2 pi k xi would not."""
    from fourierflow_amd import ops
    u, xi = _inputs(3, 70, 5, lo=-16.0, hi=16.0)
    spec = ops.point_fft2d(_dev(u, host_device, False), _dev(xi, host_device, False), 16, 16)
    ref = po.fft2d(torch.tensor(u), torch.tensor(xi), 16, 16)
    assert rel_l2(torch.view_as_real(spec).cpu().numpy(), torch.view_as_real(ref).numpy()) < 1e-5
    V = _spec(2, 3, 16, 6)
    out = ops.point_ifft2d(torch.tensor(V, dtype=torch.complex64, device=host_device), _dev(xi, host_device, False))
    assert rel_l2(out.cpu().numpy(), po.ifft2d(torch.tensor(V), torch.tensor(xi)).numpy()) < 1e-5


@pytest.mark.parametrize("kind", BACKENDS)
def test_c_abi_dxi_accumulates_and_rejects(kind):
    """ffno_nudft_points(accumulate = 1) adds its dxi to what the buffer holds (the two transforms' dxi are summed into one
    buffer); null / unsupported arguments are refused before any launch."""
    be = Backend(kind)
    lib, p = be.lib, be.ptr
    B, C, N, m = 2, 8, 90, 12
    _, xi = _inputs(C, N, 3)
    V = _spec(B, C, m, 4)
    w = np.random.default_rng(8).standard_normal((B, C, N)).astype(np.float32)
    spec = be.put(np.ascontiguousarray(np.stack([V.real, V.imag], -1)).astype(np.float32))
    x, wd = be.put(xi.astype(np.float32)), be.put(w)
    d0 = be.put(np.zeros((B, N, 2), np.float32))
    assert lib.ffno_nudft_points(p(spec), p(x), p(wd), None, p(d0), B, C, N, m, m, 1, 0, None) == 0
    base = be.get(d0).copy()
    start = np.random.default_rng(9).standard_normal((B, N, 2)).astype(np.float32)
    d1 = be.put(start)
    assert lib.ffno_nudft_points(p(spec), p(x), p(wd), None, p(d1), B, C, N, m, m, 1, 1, None) == 0
    assert rel_l2(be.get(d1), start + base) < 1e-6
    x64 = torch.tensor(xi, requires_grad=True)
    ref, = torch.autograd.grad(po.ifft2d(torch.tensor(V), x64), (x64,), torch.tensor(w, dtype=torch.float64))
    assert rel_l2(base, ref.numpy()) < 5e-5
    assert lib.ffno_nudft_points(p(spec), p(x), None, None, p(d0), B, C, N, m, m, 1, 0, None) == -1     # dxi needs w
    assert lib.ffno_nudft_points(p(spec), p(x), None, None, None, B, C, N, m, m, 1, 0, None) == -1      # nothing to write
    assert lib.ffno_nudft_modes(p(wd), p(x), p(spec), B, C, N, 17, m, 0, None) == -2                    # modes > 16
    assert lib.ffno_nudft_supported(C, 16, 16) == 1 and lib.ffno_nudft_supported(C, 16, 17) == 0


def test_point_transforms_refuse_cpu_tensors():
    """HIP only: without the emulator backend, CPU tensors raise instead of falling back to torch."""
    from fourierflow_amd import _lib, ops
    u, xi = torch.zeros(1, 3, 10), torch.zeros(1, 10, 2)
    with pytest.raises(_lib.FFNOLibraryError):
        ops.point_fft2d(u, xi, 4, 4)
    with pytest.raises(_lib.FFNOLibraryError):
        ops.point_ifft2d(torch.zeros(1, 3, 8, 4, dtype=torch.complex64), xi)
