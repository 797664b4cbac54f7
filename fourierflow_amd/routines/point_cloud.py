"""PointCloudExperiment -- counterpart of ``fourierflow.routines.PointCloudExperiment`` (reference routines/point_cloud.py:9-65):
the elasticity F-FNO (``FNOFactorizedPointCloud2D`` + ``IPhi``) or its geo-FNO baseline (``FNOPointCloud2D`` + ``IPhi``)
regressing the stress ``sigma`` at the mesh points ``xy`` from the geometry code ``rr`` under the relative-L2 loss, with the
manual optimisation step of routines/base.py:27-52.

The reference adds ``0 * loss_reg`` (IPhi on ``N`` random points against the identity, point_cloud.py:36-39): multiplied by zero
it contributes no gradient, so it is not evaluated here; ``N`` is kept as an attribute.  Validation and test use the same loss.

The optimiser step is the project's: every parameter that receives a gradient is a view into one flat fp32 buffer, one
``ffno_adamw_flat`` launch per step under the cosine-with-warm-up schedule of :class:`FFNOTrainer` (the F-FNO configs), or
``optimizer_type="adam"``: one ``ffno_adam_flat`` launch (torch.optim.Adam, L2 weight decay) under StepLR(step_size, gamma)
per EPOCH, recognised by its keyword arguments (the geo-FNO configs), exactly as StructuredMeshExperiment does.
torch.optim.Adam(W) skips parameters whose ``.grad`` is None (weight decay included), so what is registered and never used stays
out of the flat buffer and is never written: ``iphi.fc_no_code.*`` always, and the prefixes a model lists in its
``unused_parameter_prefixes`` (``ws.`` of the F-FNO; the geo-FNO uses its ``ws``).  Shared Fourier weights appear once.
"""
from typing import Optional

import torch
import torch.nn as nn

from .checkpoint import CheckpointMixin, reject_unsupported_routine_kwargs
from .optimizer import EpochEndMixin


class _AutogradEngine:
    """The engine protocol FFNOTrainer / CheckpointMixin use (n_params, param_names, param_shapes, bind, backward -> flat
    gradient, weights_changed) over a model whose forward pass is a composition of autograd ops: backward is
    ``torch.autograd.backward`` into views of the flat gradient buffer."""

    can_return_view = False

    def __init__(self, named):
        self.param_names = [n for n, _ in named]
        self.param_shapes = {n: tuple(p.shape) for n, p in named}
        self._params = [p for _, p in named]
        self._offsets, off = {}, 0
        for n, p in named:      # keyed the way CheckpointMixin looks parameters up ("model." stripped)
            self._offsets[n[len("model."):] if n.startswith("model.") else n] = off
            off += p.numel()
        self.param_shapes.update({k: self.param_shapes[("model." + k) if ("model." + k) in self.param_shapes else k]
                                  for k in self._offsets})
        self.n_params = off
        self.gflat = None

    def bind(self, views):
        self._views = views

    def backward(self, out, gy):
        p0 = self._params[0]
        if self.gflat is None or self.gflat.device != p0.device:
            self.gflat = torch.empty(self.n_params, dtype=torch.float32, device=p0.device)
        self.gflat.zero_()
        off = 0
        for p in self._params:      # autograd accumulates in place into an existing .grad
            p.grad = self.gflat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        torch.autograd.backward(out, gy)
        return self.gflat

    def weights_changed(self):
        # the optimiser kernel wrote the parameters through a raw pointer: tell everything that keys derived operands on a
        # tensor's version counter (the packed Fourier weights of ops.spectral_conv2d)
        for p in self._params:
            torch.autograd.graph.increment_version(p)


class _TrainedParameters:
    """What FFNOTrainer asks of a block: the engine and the (name, parameter) list of its flat buffer."""

    def __init__(self, routine):
        seen, named = set(), []
        skip = tuple("model." + pre for pre in routine.model.unused_parameter_prefixes) + ("iphi.fc_no_code.",)
        for n, p in routine.named_parameters():      # (shared tensors are reported once)
            if n.startswith(skip) or id(p) in seen:
                continue
            seen.add(id(p))
            named.append((n, p))
        self._named = named
        self._engine = _AutogradEngine(named)

    def engine(self):
        return self._engine

    def engine_parameters(self):
        return self._named


class PointCloudExperiment(EpochEndMixin, CheckpointMixin, nn.Module):
    def __init__(self, model: nn.Module, iphi: nn.Module, N: int = 1000, optimizer: Optional[dict] = None,
                 scheduler: Optional[dict] = None, optimizer_type: str = "adamw", **unused):
        super().__init__()
        reject_unsupported_routine_kwargs(unused)
        if optimizer_type not in ("adamw", "adam"):
            raise NotImplementedError(f"optimizer_type={optimizer_type!r}: the fused step implements AdamW and Adam")
        self.model, self.iphi, self.N, self.optimizer_type = model, iphi, N, optimizer_type
        # the F-FNO configs run cosine-with-warm-up per step, the geo-FNO baseline (FNOPointCloud2D) torch.optim.Adam + StepLR per
        # EPOCH
        self._init_optimizer(optimizer, scheduler, lr=1e-3, step_size=50, num_training_steps=10000)

    def _trainer_args(self):
        return _TrainedParameters(self), dict(decoupled=self.optimizer_type == "adamw")

    def forward(self, batch):
        return self.model(batch['xy'], code=batch['rr'], iphi=self.iphi)

    def training_step(self, batch, batch_idx: int = 0):
        tr = self.trainer()
        out = self.model(batch['xy'], code=batch['rr'], iphi=self.iphi)
        loss, gy = tr.loss_and_grad(out.detach(), batch['sigma'].contiguous(), fresh_loss=True)
        return tr.apply_gradients(tr.engine.backward(out, gy), loss, loss_is_fresh=True)

    @torch.no_grad()
    def validation_step(self, batch, batch_idx: int = 0):
        tr = self.trainer()
        out = self.model(batch['xy'], code=batch['rr'], iphi=self.iphi)
        loss, _ = tr.loss_and_grad(out, batch['sigma'].contiguous(), fresh_loss=True)
        return loss

    test_step = validation_step
