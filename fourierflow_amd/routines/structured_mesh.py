"""StructuredMeshExperiment -- counterpart of ``fourierflow.routines.StructuredMeshExperiment``
(reference routines/structured_mesh.py:8-31): plain x -> y regression of a mesh operator
(``FNOFactorizedMesh3D``) under the relative-L2 loss with the manual optimisation step of routines/base.py:27-52.
"""
from typing import Optional

import torch.nn as nn

from .checkpoint import CheckpointMixin, reject_unsupported_routine_kwargs
from .optimizer import EpochEndMixin


class StructuredMeshExperiment(EpochEndMixin, CheckpointMixin, nn.Module):
    def __init__(self, model: nn.Module, loss_scale: float = 1.0, optimizer: Optional[dict] = None,
                 scheduler: Optional[dict] = None, optimizer_type: str = "adamw", **unused):
        super().__init__()
        reject_unsupported_routine_kwargs(unused)
        if optimizer_type not in ("adamw", "adam"):
            raise NotImplementedError(f"optimizer_type={optimizer_type!r}: the fused step implements AdamW and Adam")
        self.model, self.loss_scale, self.optimizer_type = model, loss_scale, optimizer_type
        # the F-FNO configs run cosine-with-warm-up per step, the geo-FNO baselines (FNOMesh2D) torch.optim.Adam + StepLR per EPOCH
        self._init_optimizer(optimizer, scheduler, lr=1e-3, step_size=100, num_training_steps=100000)

    def _trainer_args(self):
        return self.model, dict(loss_scale=self.loss_scale, decoupled=self.optimizer_type == "adamw")

    def training_step(self, batch, batch_idx: int = 0):
        return self.trainer().train_step(batch['x'], batch['y'])

    def validation_step(self, batch, batch_idx: int = 0):
        tr = self.trainer()
        pred = tr.predict(batch['x'])
        loss, _ = tr.loss_and_grad(pred, batch['y'].contiguous())
        return loss
