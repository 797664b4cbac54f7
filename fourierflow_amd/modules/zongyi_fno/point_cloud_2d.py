"""FNOPointCloud2D -- MI355X-native mirror of ``fourierflow.modules.zongyi_fno.point_cloud_2d`` (reference
point_cloud_2d.py:155-253), the geo-FNO of Li et al. that the elasticity experiments set against the F-FNO
(experiments/elasticity/geo-fno*, geo-fno-big*).

Same constructor, parameter names / shapes / dtypes and registration order (``convs.{0..L}.weights1/2`` are complex64 in the
state_dict, stored as their ``view_as_real`` twins; ``ws.{i}`` are used here), same forward contract
``forward(u [B, N, in], code, x_in=None, x_out=None, iphi=None) -> [B, N, out]`` and full autograd in the parameters of the model
and of ``iphi``.  The forward pass is a composition of the operator-level HIP ops (fourierflow_amd/ops.py):

    xi = iphi(x, code)                                            ops.iphi_forward            (once when x_in is x_out)
    V  = mix_0(W0 . fft2d([u, 1], xi))                             ops.point_fft2d on in + 1 channels (fc0 is affine, so the
                                                                   transform of its W outputs is a [W, in + 1] mix of these),
                                                                   ops.mix_corner_modes
    uc = gelu(irfft2(V) + bs[0](grid))                             ops.modes_to_grid, ops.geofno_pointwise
    uc = gelu(irfft2(mix_i(rfft2(uc))) + ws[i-1](uc) + bs[i](grid))    ops.grid_to_mixed_modes, ops.modes_to_grid,
                                                                   ops.geofno_pointwise          (i = 1 .. L - 1)
    t  = ifft2d(mix_L(rfft2(uc)), xi)                              ops.grid_to_mixed_modes, ops.point_ifft2d
    y  = fc2(gelu(fc1(t + bs[L](x_out))))                          ops.point_head

HIP only: CPU tensors raise.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from .mesh_2d import _ComplexCornerWeights


class SpectralConv2d(_ComplexCornerWeights):
    """point_cloud_2d.py:14-34: the parameter container of one Fourier layer, two corner-block weight tensors."""

    def __init__(self, in_channels, out_channels, modes1, modes2, s1=32, s2=32):
        super().__init__(in_channels, out_channels, (modes1, modes2), 2)
        self.modes1, self.modes2, self.s1, self.s2 = modes1, modes2, s1, s2

    def forward(self, *args, **kwargs):
        raise RuntimeError("the point-cloud Fourier layers run inside FNOPointCloud2D.forward; call the model")


class FNOPointCloud2D(nn.Module):
    # registered parameters that forward never reads (PointCloudExperiment keeps those out of the optimiser): none here
    unused_parameter_prefixes = ()

    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers=4, is_mesh=True, s1=40, s2=40):
        super().__init__()
        self.modes1, self.modes2, self.width, self.is_mesh = modes1, modes2, width, is_mesh
        self.s1, self.s2, self.n_layers = s1, s2, n_layers
        self.in_channels, self.out_channels = in_channels, out_channels
        self.fc0 = nn.Linear(in_channels, width)
        self.convs = nn.ModuleList([])
        self.ws = nn.ModuleList([])
        self.bs = nn.ModuleList([])
        for i in range(n_layers + 1):
            if i in (0, n_layers):
                self.convs.append(SpectralConv2d(width, width, modes1, modes2, s1, s2))
            else:
                self.convs.append(SpectralConv2d(width, width, modes1, modes2))
        for i in range(n_layers + 1):
            self.bs.append(nn.Conv2d(2, width, 1) if i < n_layers else nn.Conv1d(2, width, 1))
        for _ in range(n_layers - 1):
            self.ws.append(nn.Conv2d(width, width, 1))
        self.fc1 = nn.Linear(width, 128)
        self.fc2 = nn.Linear(128, out_channels)

    def get_grid(self, shape, device):
        """[B, s1, s2, 2]: linspace(0, 1, s) per axis, end point included (point_cloud_2d.py:245-253)."""
        B, X, Y = shape[0], shape[1], shape[2]
        gx = torch.tensor(np.linspace(0, 1, X), dtype=torch.float).reshape(1, X, 1, 1).repeat([B, 1, Y, 1])
        gy = torch.tensor(np.linspace(0, 1, Y), dtype=torch.float).reshape(1, 1, Y, 1).repeat([B, X, 1, 1])
        return torch.cat((gx, gy), dim=-1).to(device)

    def forward(self, u, code=None, x_in=None, x_out=None, iphi=None):
        from ... import ops
        _lib.require_device_tensor(u, "FNOPointCloud2D input")
        if u.dim() != 3 or u.shape[2] != self.in_channels:
            raise ValueError(f"expected u [B, N, {self.in_channels}], got {tuple(u.shape)}")
        if self.is_mesh and x_in is None:
            x_in = u
        if self.is_mesh and x_out is None:
            x_out = u
        if x_in is None or x_out is None:
            raise ValueError("is_mesh=False needs explicit x_in and x_out")
        B, N = u.shape[:2]
        W, m1, m2, s1, s2, L = self.width, self.modes1, self.modes2, self.s1, self.s2, self.n_layers
        # the reference evaluates iphi in fft2d and again in ifft2d; on the same points that is one evaluation whose two
        # coordinate gradients autograd sums
        xi_in = x_in if iphi is None else iphi(x_in, code)
        xi_out = xi_in if x_out is x_in else (x_out if iphi is None else iphi(x_out, code))

        # layer 0: fc0 is affine in [u, 1], so fft2d(fc0(u)) = [fc0.weight | fc0.bias] . fft2d([u, 1]) -- in + 1 channels
        # through the non-uniform DFT instead of W; then the corner mix in mode space
        aug = torch.cat([u.permute(0, 2, 1), torch.ones(B, 1, N, dtype=u.dtype, device=u.device)], dim=1)
        v = torch.view_as_real(ops.point_fft2d(aug, xi_in, m1, m2))                    # [B, in + 1, 2 m1, m2, 2]
        rows = v.permute(3, 2, 0, 4, 1).reshape(-1, self.in_channels + 1)               # mode-major, channels last
        w0 = torch.cat([self.fc0.weight, self.fc0.bias[:, None]], dim=1)
        z = ops._LinearFn.apply(rows.contiguous(), w0.contiguous(), torch.zeros(W, dtype=u.dtype, device=u.device))
        z = ops.mix_corner_modes(z.view(m2, 2 * m1, B, 2, W), self.convs[0].weights1, self.convs[0].weights2, (s1, s2))
        uc = ops.geofno_pointwise(ops.modes_to_grid(z, s1, s2), self.bs[0])             # [B, s1, s2, W]
        for i in range(1, L):
            conv = self.convs[i]
            spec = ops.modes_to_grid(ops.grid_to_mixed_modes(uc, conv.weights1, conv.weights2), s1, s2)
            uc = ops.geofno_pointwise(spec, self.bs[i], uc, self.ws[i - 1])
        last = self.convs[L]
        zo = ops.grid_to_mixed_modes(uc, last.weights1, last.weights2)                   # [m2, 2 m1, B, 2, W]
        t = ops.point_ifft2d(torch.view_as_complex(zo.permute(2, 4, 1, 0, 3).contiguous()), xi_out)
        return ops.point_head(t, x_out, self.bs[L], self.fc1, self.fc2)
