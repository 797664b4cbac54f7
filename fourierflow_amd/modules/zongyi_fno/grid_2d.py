"""FNOZongyi2DBlock -- MI355X-native mirror of ``fourierflow.modules.zongyi_fno.grid_2d`` (reference grid_2d.py:16-129),
the original FNO baseline of BASELINE config 0 (experiments/torus_li/zongyi/4_layers: modes 12, width 20, 4 layers).

Same constructor signature, parameter names / shapes / registration order (state_dict compatible) and forward contract
(``{'forecast': [B, M, N, 1]}``); underneath is the HIP kernel sequence of
:class:`fourierflow_amd.engine_zongyi.ZongyiEngine`.  HIP only: CPU tensors raise.  The autograd node also returns the
INPUT gradient and several forward passes may be alive at once, which is what the 10-step rollout training of
Grid2DRolloutExperiment needs.
"""
import torch
import torch.nn as nn

from ... import _lib
from ...engine_zongyi import ZongyiEngine
from .._engine_module import EngineModule


class SpectralConv2d(nn.Module):
    """Parameter container of one layer (grid_2d.py:17-30): ``linear`` then the two corner-block weights."""

    def __init__(self, in_dim, out_dim, n_modes, resdiual=True, dropout=0.1):
        super().__init__()
        self.in_dim, self.out_dim, self.n_modes, self.residual = in_dim, out_dim, n_modes, resdiual
        self.linear = nn.Linear(in_dim, out_dim)
        self.fourier_weight = nn.ParameterList(
            [nn.Parameter(torch.empty(in_dim, out_dim, n_modes, n_modes, 2)) for _ in range(2)])
        for param in self.fourier_weight:
            nn.init.xavier_normal_(param, gain=1 / (in_dim * out_dim))      # grid_2d.py:29-30

    def forward(self, x):
        raise RuntimeError("layers of FNOZongyi2DBlock run inside the block's fused HIP pass; call the block")


class FNOZongyi2DBlock(EngineModule, nn.Module):
    def __init__(self, modes1, modes2, width, input_dim=12, dropout=0.1, n_layers=4, residual=False, conv_residual=True):
        super().__init__()
        if modes1 != modes2:
            raise NotImplementedError("modes1 != modes2: the reference itself only uses modes1 (grid_2d.py:111)")
        self.modes1, self.modes2, self.width, self.input_dim = modes1, modes2, width, input_dim
        self.n_layers, self.residual, self.conv_residual = n_layers, residual, conv_residual
        self.in_proj = nn.Linear(input_dim, width)
        self.spectral_layers = nn.ModuleList([
            SpectralConv2d(in_dim=width, out_dim=width, n_modes=modes1, resdiual=conv_residual, dropout=dropout)
            for _ in range(n_layers)])
        self.feedforward = nn.Sequential(nn.Linear(width, 128), nn.ReLU(inplace=True), nn.Linear(128, 1))
        self.weights_frozen = False              # True: the padded / packed weights of the last pass are still valid
        self.fused_grad_accumulation = False     # True: parameter gradients accumulate in engine().gflat, .grad stays None
        self.max_live_passes = 16       # forward passes that may await their backward at once (rollout: n_steps)
        self._tickets, self._cursor, self._ticket = {}, 0, 0

    def engine(self) -> ZongyiEngine:
        if self._engine is None:
            self._engine = ZongyiEngine(modes=self.modes1, width=self.width, input_dim=self.input_dim, n_layers=self.n_layers,
                                        residual=self.residual, conv_residual=self.conv_residual)
        return self._engine

    def _next_slot(self):
        slot = self._cursor % self.max_live_passes
        self._cursor += 1
        self._ticket += 1
        self._tickets[slot] = self._ticket
        return slot

    # -- several passes alive at once: a slot and a ticket per saved pass instead of the generation count -----------------
    def _run_forward(self, eng, x, save):
        slot = self._next_slot() if save else 0
        y = eng.forward(x, save, slot=slot, n_slots=self.max_live_passes, weights_ready=self.weights_frozen)
        return y, (slot, self._tickets[slot] if save else None)

    def _run_backward(self, eng, token, gy, need_dx):
        slot, ticket = token
        if self._tickets[slot] != ticket:
            raise RuntimeError(f"FNOZongyi2DBlock: more than max_live_passes={self.max_live_passes} forward passes were "
                               "alive at once; raise module.max_live_passes")
        if self.fused_grad_accumulation:      # the routine reads eng.gflat after the whole graph ran (eng.zero_grad() first)
            res = eng.backward(gy, slot=slot, need_dx=need_dx, accumulate=True)
            return None, res[1] if need_dx else None
        return eng.backward(gy, slot=slot, need_dx=True)

    def forward(self, x, **kwargs):
        # x.shape == [n_batches, *dim_sizes, input_size]
        _lib.require_device_tensor(x, "FNOZongyi2DBlock input")
        return {'forecast': self._apply_engine(x)}
