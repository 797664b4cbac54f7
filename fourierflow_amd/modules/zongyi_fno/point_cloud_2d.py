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
import torch

from ... import ops
from .._point_cloud import PointCloudLayer, PointCloudModel
from .mesh_2d import _ComplexCornerWeights


class SpectralConv2d(PointCloudLayer, _ComplexCornerWeights):
    """point_cloud_2d.py:14-34: the parameter container of one Fourier layer, two corner-block weight tensors."""

    model_name = "FNOPointCloud2D"

    def __init__(self, in_channels, out_channels, modes1, modes2, s1=32, s2=32):
        super().__init__(in_channels, out_channels, (modes1, modes2), 2)
        self.modes1, self.modes2, self.s1, self.s2 = modes1, modes2, s1, s2


class FNOPointCloud2D(PointCloudModel):
    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers=4, is_mesh=True, s1=40, s2=40):
        super().__init__(modes1, modes2, width, in_channels, out_channels, n_layers, is_mesh, s1, s2)
        for i in range(n_layers + 1):
            if i in (0, n_layers):
                self.convs.append(SpectralConv2d(width, width, modes1, modes2, s1, s2))
            else:
                self.convs.append(SpectralConv2d(width, width, modes1, modes2))
        self._register_tail(grid_biases=n_layers)

    def forward(self, u, code=None, x_in=None, x_out=None, iphi=None):
        x_out, xi_in, xi_out = self._points(u, code, x_in, x_out, iphi)
        s1, s2, L = self.s1, self.s2, self.n_layers
        # layer 0: the lifted spectrum, then the corner mix in mode space
        z = ops.mix_corner_modes(self._lifted_corner_modes(u, xi_in), self.convs[0].weights1, self.convs[0].weights2, (s1, s2))
        uc = ops.geofno_pointwise(ops.modes_to_grid(z, s1, s2), self.bs[0])             # [B, s1, s2, W]
        for i in range(1, L):
            conv = self.convs[i]
            spec = ops.modes_to_grid(ops.grid_to_mixed_modes(uc, conv.weights1, conv.weights2), s1, s2)
            uc = ops.geofno_pointwise(spec, self.bs[i], uc, self.ws[i - 1])
        last = self.convs[L]
        zo = ops.grid_to_mixed_modes(uc, last.weights1, last.weights2)                   # [m2, 2 m1, B, 2, W]
        t = ops.point_ifft2d(torch.view_as_complex(zo.permute(2, 4, 1, 0, 3).contiguous()), xi_out)
        return self._head(t, x_out)
