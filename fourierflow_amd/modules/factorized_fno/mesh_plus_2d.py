"""FNOFullyFactorizedMesh2D -- MI355X-native mirror of ``fourierflow.modules.factorized_fno.mesh_plus_2d`` (reference
mesh_plus_2d.py:14-280): the elasticity F-FNO with the factorisation carried to the point cloud itself.  Features move between
the N mesh points and ``modes2 + modes1`` one-dimensional modes, one set per coordinate, instead of a block of
``2 modes1 modes2`` two-dimensional ones.

Same constructor, parameter names / shapes / dtypes and registration order (the never-read ``ws.{i}`` and
``convs.{n_layers}.backcast_ff.*`` included), same forward contract ``forward(u [B, N, in], code, x_in=None, x_out=None, iphi)
-> [B, N, out]`` and full autograd in the parameters of the model and of ``iphi``.  Coordinate 0 of ``iphi``'s output pairs with
the last grid axis (y, ``modes2``, ``fourier_weight[0]``), coordinate 1 with the first (x, ``modes1``, ``fourier_weight[1]``)
(mesh_plus_2d.py:121-140).  The forward pass is a composition of the operator-level HIP ops (fourierflow_amd/ops.py), S = s1 = s2:

    xi = iphi(x, code)                                            ops.iphi_forward            (once when x_in is x_out)
    A  = axis_fft([u, 1], xi)                                      ops.point_axis_fft on in + 1 channels: fc0 is affine, so the
                                                                   transform of its W outputs is a [W, in + 1] mix of these
    s  = h(x) + g(y),  g = irfft(mix_y(A_y), n=S), h likewise      per-mode channel mix (complex einsum), ops.axis_modes_to_grid
    uc = backcast_0(s) + G,  G = bs[0](grid)                       ops.feedforward; G once per forward (pointwise linear)
    uc = uc + backcast_i(F_i(uc)) + G      (middle layers)         ops.spectral_conv2d + ops.feedforward (residual fused)
    T  = mix(rfft_y(sum_x uc)), mix(rfft_x(sum_y uc))              ops.grid_to_axis_modes, per-mode channel mix
    t  = Re sum_j T_y e(j xi_0) + Re sum_k T_x e(k xi_1)           ops.point_axis_ifft
    y  = fc2(gelu(fc1(t + bs[1](x_out))))                          ops.point_head

The reference's `irfft(n=s1, dim=-1)` / `irfft(n=s2, dim=-2)` (:78, :106) mix the two grid axes: it fails for s1 != s2, and so
does this constructor.  HIP only: CPU tensors raise.
"""
import torch
import torch.nn as nn

from ... import _lib, ops
from .._point_cloud import PointCloudLayer, PointCloudModel
from ..feedforward import FeedForward


class SpectralConv2d(PointCloudLayer, nn.Module):
    """mesh_plus_2d.py:14-39: the parameter container of one layer -- ``fourier_weight`` = [modes2 weight, modes1 weight],
    each [in, out, n_modes, 2], and its ``backcast_ff``."""

    model_name = "FNOFullyFactorizedMesh2D"

    def __init__(self, in_dim, out_dim, m1, m2, backcast_ff, fourier_weight, factor, ff_weight_norm, n_ff_layers, layer_norm,
                 dropout, s1, s2):
        super().__init__()
        if in_dim != out_dim:
            raise NotImplementedError("in_dim != out_dim is not used by the fully factorised F-FNO")
        self.in_dim, self.out_dim, self.m1, self.m2, self.s1, self.s2 = in_dim, out_dim, m1, m2, s1, s2
        self.fourier_weight = fourier_weight
        if not self.fourier_weight:
            self.fourier_weight = nn.ParameterList([])
            for n_modes in (m2, m1):
                param = nn.Parameter(torch.empty(in_dim, out_dim, n_modes, 2))
                nn.init.xavier_normal_(param)
                self.fourier_weight.append(param)
        self.backcast_ff = backcast_ff
        if not self.backcast_ff:
            self.backcast_ff = FeedForward(out_dim, factor, ff_weight_norm, n_ff_layers, layer_norm, dropout, general_ok=True)

    def mode_weights(self):
        """complex [in, out, modes2 + modes1]: the y weights, then the x weights"""
        return torch.cat([torch.view_as_complex(self.fourier_weight[0]), torch.view_as_complex(self.fourier_weight[1])], dim=-1)


class FNOFullyFactorizedMesh2D(PointCloudModel):
    iphi_optional = False      # the reference calls iphi unconditionally (mesh_plus_2d.py:123, :149)

    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers=4, is_mesh=True, s1=40, s2=40):
        if s1 != s2:
            raise ValueError(f"FNOFullyFactorizedMesh2D: s1 = {s1} != s2 = {s2}; the reference fails there (its irfft(n=s1, dim=-1) "
                             "mixes the two grid axes), only square latent grids are defined")
        if modes1 < 1 or modes2 < 1 or max(modes1, modes2) > s1 // 2 + 1:
            raise ValueError(f"FNOFullyFactorizedMesh2D: modes ({modes1}, {modes2}) must lie in 1 .. s1 // 2 + 1 = {s1 // 2 + 1}")
        if n_layers < 1:
            raise ValueError("FNOFullyFactorizedMesh2D: n_layers must be at least 1")
        super().__init__(modes1, modes2, width, in_channels, out_channels, n_layers, is_mesh, s1, s2)
        # never used by forward (mesh_plus_2d.py:254-257); kept for state-dict parity
        self.unused_parameter_prefixes = ("ws.", f"convs.{n_layers}.backcast_ff.")
        for _ in range(n_layers + 1):
            self.convs.append(SpectralConv2d(in_dim=width, out_dim=width, m1=modes1, m2=modes2, backcast_ff=None,
                                             fourier_weight=None, factor=2, ff_weight_norm=True, n_ff_layers=2, layer_norm=False,
                                             dropout=0.0, s1=s1, s2=s2))
        self._register_tail()

    def _check_kernel_set(self):
        W, m1, m2 = self.width, self.modes1, self.modes2
        if W not in (32, 64):
            raise ValueError(f"width {W} is outside the compiled channel tiles (32 / 64)")
        if not _lib.get_lib().ffno_nudft_axis_supported(W, m1, m2):
            raise ValueError(f"modes ({m1}, {m2}) are outside the compiled set of the per-axis non-uniform DFT (1..32 each)")

    def forward(self, u, code=None, x_in=None, x_out=None, iphi=None):
        x_out, xi_in, xi_out = self._points(u, code, x_in, x_out, iphi)
        m1, m2, S, L = self.modes1, self.modes2, self.s1, self.n_layers
        # layer 0: the mix of the affine lift is folded into the layer's mode weights
        aug, w0 = self._lift(u)                                                           # [B, in + 1, N], [W, in + 1]
        a = ops.point_axis_fft(aug, xi_in, m1, m2)                                        # [B, in + 1, m2 + m1]
        first = self.convs[0]
        folded = torch.einsum("ia,iok->aok", w0.to(torch.complex64), first.mode_weights())
        s = ops.axis_modes_to_grid(torch.einsum("bak,aok->bok", a, folded), S, modes2=m2)  # [B, S, S, W] = h(x) + g(y)
        G = self._grid_bias(u.device)
        ff = first.backcast_ff
        uc = ops.feedforward(s, None, ff.layers[0][0], ff.layers[1][0]) + G              # no residual in this layer
        mm = max(m1, m2)
        for i in range(1, L):
            conv = self.convs[i]
            ff = conv.backcast_ff
            # ops.spectral_conv2d takes one mode count: the shorter weight zero-padded to the longer gives the identical result
            w_y, w_x = (nn.functional.pad(w, (0, 0, 0, mm - w.shape[2])) if w.shape[2] < mm else w for w in conv.fourier_weight)
            uc = ops.feedforward(ops.spectral_conv2d(uc, w_y, w_x, mm), uc, ff.layers[0][0], ff.layers[1][0]) + G
        T = torch.einsum("bik,iok->bok", ops.grid_to_axis_modes(uc, m1, m2), self.convs[L].mode_weights())
        t = ops.point_axis_ifft(T, xi_out, modes2=m2)                                     # [B, W, N]
        return self._head(t, x_out)
