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
import torch

from ... import ops
from .._point_cloud import PointCloudLayer, PointCloudModel
from ..zongyi_fno.mesh_2d import _ComplexCornerWeights
from .grid_2d import SpectralConv2d as FactorizedSpectralConv2d
from .grid_2d import _fourier_weights


class SpectralConv2d(PointCloudLayer, _ComplexCornerWeights):
    """point_cloud_2d.py:16-37: the non-uniform Fourier layer's parameter container; ``transform=False`` has no weights."""

    model_name = "FNOFactorizedPointCloud2D"

    def __init__(self, in_channels, out_channels, modes1, modes2, s1=32, s2=32, transform=True):
        super().__init__(in_channels, out_channels, (modes1, modes2), 2 if transform else 0)
        self.modes1, self.modes2, self.s1, self.s2 = modes1, modes2, s1, s2


class FNOFactorizedPointCloud2D(PointCloudModel):
    unused_parameter_prefixes = ("ws.",)      # never used by forward (point_cloud_2d.py:257); kept for state-dict parity

    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers=4, is_mesh=True, s1=40, s2=40,
                 share_weight=False):
        super().__init__(modes1, modes2, width, in_channels, out_channels, n_layers, is_mesh, s1, s2)
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
        self._register_tail()

    def forward(self, u, code=None, x_in=None, x_out=None, iphi=None):
        x_out, xi_in, xi_out = self._points(u, code, x_in, x_out, iphi)
        uc = ops.modes_to_grid(self._lifted_corner_modes(u, xi_in), self.s1, self.s2)    # [B, s1, s2, W]
        G = self._grid_bias(u.device)
        uc = uc + G
        for i in range(1, self.n_layers):
            conv = self.convs[i]
            ff = conv.backcast_ff
            uc = ops.feedforward(conv.forward_fourier(uc), uc, ff.layers[0][0], ff.layers[1][0]) + G
        last = self.convs[self.n_layers]
        zo = ops.grid_to_mixed_modes(uc, last.weights1, last.weights2)                   # [m2, 2 m1, B, 2, W]
        t = ops.point_ifft2d(torch.view_as_complex(zo.permute(2, 4, 1, 0, 3).contiguous()), xi_out)
        return self._head(t, x_out)
