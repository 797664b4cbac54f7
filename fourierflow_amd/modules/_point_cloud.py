"""What the three point-cloud models of the elasticity experiments share (``FNOFactorizedPointCloud2D``, ``FNOPointCloud2D``,
``FNOFullyFactorizedMesh2D``): the parameter tree around their Fourier layers, the latent grid, the preface of ``forward``
(checks, point defaults, one ``iphi`` evaluation on shared points), the affine lift through the non-uniform DFT and the head.

A model derives from :class:`PointCloudModel`, appends its layers to ``self.convs`` between ``super().__init__`` and
``self._register_tail``, and writes in ``forward`` only what lies between ``self._points`` and ``self._head``.
"""
import torch
import torch.nn as nn

from .. import _lib, ops


class PointCloudLayer:
    """Mixin of the per-layer parameter containers: they hold parameters, the arithmetic is the model's."""

    model_name = "the model"

    def forward(self, *args, **kwargs):
        raise RuntimeError(f"the point-cloud Fourier layers run inside {self.model_name}.forward; call the model")


class PointCloudModel(nn.Module):
    # registered parameters that forward never reads (PointCloudExperiment keeps those out of the optimiser)
    unused_parameter_prefixes = ()
    # the reference calls iphi unconditionally in some models; those refuse iphi=None
    iphi_optional = True

    def __init__(self, modes1, modes2, width, in_channels, out_channels, n_layers, is_mesh, s1, s2):
        super().__init__()
        self.modes1, self.modes2, self.width, self.is_mesh = modes1, modes2, width, is_mesh
        self.s1, self.s2, self.n_layers = s1, s2, n_layers
        self.in_channels, self.out_channels = in_channels, out_channels
        self.fc0 = nn.Linear(in_channels, width)
        self.convs = nn.ModuleList([])
        self.ws = nn.ModuleList([])
        self.bs = nn.ModuleList([])

    def _register_tail(self, grid_biases=1):
        """What the reference registers after its layers, in its order: ``bs`` (``grid_biases`` on the latent grid, then the one
        on the output points), the ``ws`` (read by the geo-FNO only; kept everywhere for state-dict parity), fc1, fc2."""
        for _ in range(grid_biases):
            self.bs.append(nn.Conv2d(2, self.width, 1))
        self.bs.append(nn.Conv1d(2, self.width, 1))
        for _ in range(self.n_layers - 1):
            self.ws.append(nn.Conv2d(self.width, self.width, 1))
        self.fc1 = nn.Linear(self.width, 128)
        self.fc2 = nn.Linear(128, self.out_channels)

    def get_grid(self, shape, device):
        """[B, s1, s2, 2]: float32(np.linspace(0, 1, s)) per axis, end point included (reference point_cloud_2d.py:272-280,
        zongyi_fno/point_cloud_2d.py:245-253, mesh_plus_2d.py:272-280), from the tables ops keeps per (s1, s2, device)."""
        B, X, Y = shape[0], shape[1], shape[2]
        return ops.latent_grid(X, Y, device).view(1, X, Y, 2).repeat([B, 1, 1, 1])

    def _check_kernel_set(self):
        """Refuse a configuration outside the compiled kernels before anything is launched (where no op below does)."""

    def _points(self, u, code, x_in, x_out, iphi):
        """The preface of forward -> (x_out, xi_in, xi_out): u [B, N, in] on the device, the points default to u on a mesh, and
        the deformed coordinates of both point sets."""
        _lib.require_device_tensor(u, f"{type(self).__name__} input")
        if u.dim() != 3 or u.shape[2] != self.in_channels:
            raise ValueError(f"expected u [B, N, {self.in_channels}], got {tuple(u.shape)}")
        if iphi is None and not self.iphi_optional:
            raise ValueError(f"{type(self).__name__} needs iphi: the reference calls it unconditionally")
        if self.is_mesh and x_in is None:
            x_in = u
        if self.is_mesh and x_out is None:
            x_out = u
        if x_in is None or x_out is None:
            raise ValueError("is_mesh=False needs explicit x_in and x_out")
        self._check_kernel_set()
        # the reference evaluates iphi in the forward transform and again in the inverse; on the same points (the same tensor)
        # that is one evaluation whose two coordinate gradients autograd sums
        xi_in = x_in if iphi is None else iphi(x_in, code)
        xi_out = xi_in if x_out is x_in else (x_out if iphi is None else iphi(x_out, code))
        return x_out, xi_in, xi_out

    def _lift(self, u):
        """fc0 is affine in [u, 1], so a linear transform of fc0(u) is [fc0.weight | fc0.bias] applied to the transform of
        [u, 1] -- in + 1 channels through the non-uniform DFT instead of W: -> (aug [B, in + 1, N], w0 [W, in + 1])."""
        B, N = u.shape[:2]
        aug = torch.cat([u.permute(0, 2, 1), torch.ones(B, 1, N, dtype=u.dtype, device=u.device)], dim=1)
        return aug, torch.cat([self.fc0.weight, self.fc0.bias[:, None]], dim=1)

    def _lifted_corner_modes(self, u, xi_in):
        """fft2d(fc0(u), xi_in) restricted to the corner modes, mode-major: z [m2, 2 m1, B, 2, W]."""
        aug, w0 = self._lift(u)
        v = torch.view_as_real(ops.point_fft2d(aug, xi_in, self.modes1, self.modes2))    # [B, in + 1, 2 m1, m2, 2]
        rows = v.permute(3, 2, 0, 4, 1).reshape(-1, self.in_channels + 1)                 # mode-major, channels last
        return ops.linear(rows, w0).view(self.modes2, 2 * self.modes1, u.shape[0], 2, self.width)

    def _grid_bias(self, device):
        """G = bs[0](grid) [1, s1, s2, W]: pointwise linear on the latent grid's coordinates, once per forward."""
        s1, s2, W = self.s1, self.s2, self.width
        return ops.linear(ops.latent_grid(s1, s2, device), self.bs[0].weight.reshape(W, 2), self.bs[0].bias).view(1, s1, s2, W)

    def _head(self, t, x_out):
        """y = fc2(gelu(fc1(t + bs[-1](x_out)))): t [B, W, N] channel-major -> [B, N, out]."""
        return ops.point_head(t, x_out, self.bs[-1], self.fc1, self.fc2)
