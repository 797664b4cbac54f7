"""FNOMesh2D -- MI355X-native mirror of ``fourierflow.modules.zongyi_fno.mesh_2d`` (reference mesh_2d.py:14-106), the
geo-FNO baseline of the airfoil / pipe experiments (experiments/{airfoil,pipe}/geo-fno*).

Same constructor, parameter names / shapes / dtypes and registration order -- ``convs.{i}.weights1/2`` are complex64
``[in, out, modes1, modes2]`` in the state_dict exactly like the reference's (they are STORED as their ``view_as_real``
twins so that one flat fp32 buffer can hold every parameter for the fused optimiser) -- and the same forward contract
(``x [B, X, Y, 2] -> [B, X, Y, 1]``).  Underneath: :class:`fourierflow_amd.engine_geofno.GeoFNO2DEngine`.  HIP only.
"""
import torch
import torch.nn as nn

from ... import _lib
from ...engine_geofno import GeoFNO2DEngine
from .._engine_module import EngineModule


class _ComplexCornerWeights(nn.Module):
    """Parameter container of one Fourier layer: ``weights1..n``, complex64 ``[in, out, *modes]`` in the state_dict, stored as
    their ``view_as_real`` twins."""

    def __init__(self, in_channels, out_channels, modes, n_weights):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.scale = 1 / (in_channels * out_channels)
        self._names = tuple(f"weights{j}" for j in range(1, n_weights + 1))
        for name in self._names:       # scale * torch.rand(..., dtype=cfloat): real and imaginary parts U[0, 1)
            setattr(self, name, nn.Parameter(self.scale * torch.rand(in_channels, out_channels, *modes, 2)))
        self._register_state_dict_hook(self._complex_out)
        self._register_load_state_dict_pre_hook(self._complex_in)

    @staticmethod
    def _complex_out(module, state_dict, prefix, local_metadata):
        for name in module._names:
            state_dict[prefix + name] = torch.view_as_complex(state_dict[prefix + name].contiguous())

    def _complex_in(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for name in self._names:
            t = state_dict.get(prefix + name)
            if t is not None and t.is_complex():
                state_dict[prefix + name] = torch.view_as_real(t.to(torch.complex64))

    def forward(self, x):
        raise RuntimeError("Fourier layers of FNOMesh2D / FNOMesh3D run inside the model's fused HIP pass; call the model")


class SpectralConv2d(_ComplexCornerWeights):
    """mesh_2d.py:15-32: two corner-block weight tensors [in, out, modes1, modes2]."""

    def __init__(self, in_channels, out_channels, modes1, modes2):
        super().__init__(in_channels, out_channels, (modes1, modes2), 2)
        self.modes1, self.modes2 = modes1, modes2


class _GeoMeshModule(EngineModule):
    """The GeoFNO engines take no dropout switch and compute no input gradient."""

    def _run_forward(self, eng, x, save):
        return eng.forward(x, save), self._new_pass()

    def _run_backward(self, eng, token, gy, need_dx):
        if need_dx:
            # the reference modules are ordinary autograd modules and would propagate dL/dx; this operator's kernels stop at
            # the lift's parameter gradients -- fail loudly instead of silently training upstream parameters without that term
            raise RuntimeError(f"{type(self).__name__}: the gradient with respect to the INPUT tensor is not computed by the "
                               "gfx950 kernel set (feed it a tensor that does not require grad)")
        self._check_latest(token)
        return eng.backward(gy), None


class FNOMesh2D(_GeoMeshModule, nn.Module):
    def __init__(self, modes1, modes2, width, n_layers):
        super().__init__()
        self.modes1, self.modes2, self.width, self.n_layers = modes1, modes2, width, n_layers
        self.padding = 8
        self.input_dim = 4                               # (mesh x, mesh y) + the two grid channels (mesh_2d.py:62,79-80)
        self.fc0 = nn.Linear(4, width)
        self.convs = nn.ModuleList([SpectralConv2d(width, width, modes1, modes2) for _ in range(n_layers)])
        self.ws = nn.ModuleList([nn.Conv2d(width, width, 1) for _ in range(n_layers)])
        self.fc1 = nn.Linear(width, 128)
        self.fc2 = nn.Linear(128, 1)

    def engine(self) -> GeoFNO2DEngine:
        if self._engine is None:
            self._engine = GeoFNO2DEngine(modes1=self.modes1, modes2=self.modes2, width=self.width, n_layers=self.n_layers)
        return self._engine

    def get_grid(self, shape, device):
        B, X, Y = shape[0], shape[1], shape[2]
        gx = torch.linspace(0, 1, X, device=device).reshape(1, X, 1, 1).expand(B, X, Y, 1)
        gy = torch.linspace(0, 1, Y, device=device).reshape(1, 1, Y, 1).expand(B, X, Y, 1)
        return torch.cat((gx, gy), dim=-1)

    def prepare_input(self, x):
        return torch.cat((x, self.get_grid(x.shape, x.device)), dim=-1).contiguous()

    def forward(self, x):
        _lib.require_device_tensor(x, "FNOMesh2D input")
        return self._apply_engine(self.prepare_input(x))
