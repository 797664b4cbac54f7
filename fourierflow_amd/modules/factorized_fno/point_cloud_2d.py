"""FNOFactorizedPointCloud2D -- MI355X-native mirror of ``fourierflow.modules.factorized_fno.point_cloud_2d`` (reference
point_cloud_2d.py:162-280), the F-FNO of the elasticity experiments (experiments/elasticity/ffno*).

Same constructor, parameter names / shapes / dtypes and registration order (the unused ``ws.{i}`` included;
``convs.{n_layers}.weights1/2`` are complex64 in the state_dict, stored as their ``view_as_real`` twins), same forward
contract ``forward(u [B, N, 2], code, x_in=None, x_out=None, iphi=None) -> [B, N, out]`` and full autograd in the parameters
of the model and of ``iphi``.  The forward pass is a composition of the operator-level HIP ops (fourierflow_amd/ops.py):

    xi = iphi(x, code)                                            ops.iphi_forward            (once when x_in is x_out)
    V  = W0 . fft2d([u, 1], xi)                                    ops.point_fft2d on in + 1 channels: fc0 is affine, so the
                                                                   transform of its W outputs is a [W, in + 1] mix of these
    uc = irfft2(V) + G,  G = bs[0](grid)                           ops.modes_to_grid; G once per forward (pointwise linear)
    uc = uc + backcast_i(uc) + G      (middle layers)              ops.spectral_conv2d + ops.feedforward (residual fused)
    t  = ifft2d(mix(rfft2(uc)), xi)                                ops.grid_to_mixed_modes, ops.point_ifft2d
    y  = fc2(gelu(fc1(t + bs[1](x_out))))                          ops.point_head

HIP only: CPU tensors raise.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ..zongyi_fno.mesh_2d import _ComplexCornerWeights
from .grid_2d import SpectralConv2d as FactorizedSpectralConv2d
from .grid_2d import _fourier_weights


class SpectralConv2d(_ComplexCornerWeights):
    """point_cloud_2d.py:16-37: the non-uniform Fourier layer's parameter container; ``transform=False`` has no weights."""

    def __init__(self, in_channels, out_channels, modes1, modes2, s1=32, s2=32, transform=True):
        super().__init__(in_channels, out_channels, (modes1, modes2), 2 if transform else 0)
        self.modes1, self.modes2, self.s1, self.s2 = modes1, modes2, s1, s2

    def forward(self, *args, **kwargs):
        raise RuntimeError("the point-cloud Fourier layers run inside FNOFactorizedPointCloud2D.forward; call the model")


class FNOFactorizedPointCloud2D(nn.Module):
    # registered parameters that forward never reads (PointCloudExperiment keeps those out of the optimiser)
    unused_parameter_prefixes = ("ws.",)

    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers=4, is_mesh=True, s1=40, s2=40,
                 share_weight=False):
        super().__init__()
        self.modes1, self.modes2, self.width, self.is_mesh = modes1, modes2, width, is_mesh
        self.s1, self.s2, self.n_layers = s1, s2, n_layers
        self.in_channels, self.out_channels = in_channels, out_channels
        self.fc0 = nn.Linear(in_channels, width)
        self.convs = nn.ModuleList([])
        self.ws = nn.ModuleList([])
        self.bs = nn.ModuleList([])
        self.fourier_weight = None
        if share_weight:
            self.fourier_weight = _fourier_weights(width, width, modes1)
        for i in range(n_layers + 1):
            if i == 0:
                conv = SpectralConv2d(width, width, modes1, modes2, s1, s2, transform=False)
            elif i == n_layers:
                conv = SpectralConv2d(width, width, modes1, modes2, s1, s2)
            else:
                conv = FactorizedSpectralConv2d(in_dim=width, out_dim=width, n_modes=modes1, forecast_ff=None, backcast_ff=None,
                                                fourier_weight=self.fourier_weight, factor=2, ff_weight_norm=True,
                                                n_ff_layers=2, layer_norm=False, use_fork=False, dropout=0.0, mode='full')
            self.convs.append(conv)
        self.bs.append(nn.Conv2d(2, width, 1))
        self.bs.append(nn.Conv1d(2, width, 1))
        for _ in range(n_layers - 1):      # never used by forward (point_cloud_2d.py:257); kept for state-dict parity
            self.ws.append(nn.Conv2d(width, width, 1))
        self.fc1 = nn.Linear(width, 128)
        self.fc2 = nn.Linear(128, out_channels)

    def get_grid(self, shape, device):
        """[B, s1, s2, 2]: linspace(0, 1, s) per axis, end point included (point_cloud_2d.py:272-280)."""
        B, X, Y = shape[0], shape[1], shape[2]
        gx = torch.tensor(np.linspace(0, 1, X), dtype=torch.float).reshape(1, X, 1, 1).repeat([B, 1, Y, 1])
        gy = torch.tensor(np.linspace(0, 1, Y), dtype=torch.float).reshape(1, 1, Y, 1).repeat([B, X, 1, 1])
        return torch.cat((gx, gy), dim=-1).to(device)

    def forward(self, u, code=None, x_in=None, x_out=None, iphi=None):
        from ... import ops
        _lib.require_device_tensor(u, "FNOFactorizedPointCloud2D input")
        if u.dim() != 3 or u.shape[2] != self.in_channels:
            raise ValueError(f"expected u [B, N, {self.in_channels}], got {tuple(u.shape)}")
        if self.is_mesh and x_in is None:
            x_in = u
        if self.is_mesh and x_out is None:
            x_out = u
        if x_in is None or x_out is None:
            raise ValueError("is_mesh=False needs explicit x_in and x_out")
        B, N = u.shape[:2]
        W, m1, m2, s1, s2 = self.width, self.modes1, self.modes2, self.s1, self.s2
        # the reference evaluates iphi in fft2d and again in ifft2d; on the same points that is one evaluation whose two
        # coordinate gradients autograd sums
        xi_in = x_in if iphi is None else iphi(x_in, code)
        xi_out = xi_in if x_out is x_in else (x_out if iphi is None else iphi(x_out, code))

        # layer 0: fc0 is affine in [u, 1], so fft2d(fc0(u)) = [fc0.weight | fc0.bias] . fft2d([u, 1]) -- in + 1 channels
        # through the non-uniform DFT instead of W
        aug = torch.cat([u.permute(0, 2, 1), torch.ones(B, 1, N, dtype=u.dtype, device=u.device)], dim=1)
        v = torch.view_as_real(ops.point_fft2d(aug, xi_in, m1, m2))                    # [B, in + 1, 2 m1, m2, 2]
        rows = v.permute(3, 2, 0, 4, 1).reshape(-1, self.in_channels + 1)               # mode-major, channels last
        w0 = torch.cat([self.fc0.weight, self.fc0.bias[:, None]], dim=1)
        z = ops._LinearFn.apply(rows.contiguous(), w0.contiguous(), torch.zeros(W, dtype=u.dtype, device=u.device))
        uc = ops.modes_to_grid(z.view(m2, 2 * m1, B, 2, W), s1, s2)                      # [B, s1, s2, W]
        grid = self.get_grid([1, s1, s2], u.device).reshape(s1 * s2, 2)
        G = ops._LinearFn.apply(grid, self.bs[0].weight.reshape(W, 2).contiguous(), self.bs[0].bias).view(1, s1, s2, W)
        uc = uc + G
        for i in range(1, self.n_layers):
            conv = self.convs[i]
            ff = conv.backcast_ff
            uc = ops.feedforward(conv.forward_fourier(uc), uc, ff.layers[0][0], ff.layers[1][0]) + G
        last = self.convs[self.n_layers]
        zo = ops.grid_to_mixed_modes(uc, last.weights1, last.weights2)                   # [m2, 2 m1, B, 2, W]
        t = ops.point_ifft2d(torch.view_as_complex(zo.permute(2, 4, 1, 0, 3).contiguous()), xi_out)
        return ops.point_head(t, x_out, self.bs[1], self.fc1, self.fc2)
