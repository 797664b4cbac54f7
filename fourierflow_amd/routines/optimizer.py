"""The optimiser / scheduler block of the routines: the lazily built ``FFNOTrainer``, its keyword arguments from the config's
``optimizer`` and ``scheduler`` sections over the routine's own defaults, and the epoch counter that StepLR reads.

The F-FNO configs run cosine-with-warm-up per step (FFNOTrainer's own schedule); the baselines (FNOZongyi2DBlock, FNOMesh2D,
FNOPointCloud2D) run ``torch.optim.lr_scheduler.StepLR(step_size, gamma)`` per EPOCH -- recognised by its keyword arguments.
"""
from __future__ import annotations

from typing import Optional

from ..trainer import FFNOTrainer


class OptimizerMixin:
    """``trainer()`` and ``current_epoch``.  A routine calls ``_init_optimizer`` in its constructor and, unless it trains
    ``self.conv`` with the trainer's defaults, overrides ``_trainer_args``."""

    def _init_optimizer(self, optimizer: Optional[dict], scheduler: Optional[dict], *, lr: float, step_size: int,
                        num_training_steps: Optional[int] = None):
        """`lr`, StepLR's `step_size` and the cosine schedule's `num_training_steps` are the routine's own defaults; a routine
        without a cosine schedule (num_training_steps None) always runs StepLR."""
        self._opt_kw = dict(lr=lr, weight_decay=1e-4)
        self._opt_kw.update(optimizer or {})
        self._step_lr = num_training_steps is None or (scheduler is not None and "step_size" in scheduler)
        self._sch_kw = dict(step_size=step_size, gamma=0.5) if self._step_lr else \
            dict(num_warmup_steps=500, num_training_steps=num_training_steps, num_cycles=0.5)
        self._sch_kw.update(scheduler or {})
        self.current_epoch = 0
        self._trainer: Optional[FFNOTrainer] = None

    def _trainer_args(self):
        """(what FFNOTrainer is built on, its keyword arguments beside the optimiser's and the scheduler's)."""
        return self.conv, {}

    def trainer(self) -> FFNOTrainer:
        if self._trainer is None:
            block, kw = self._trainer_args()
            self._trainer = tr = FFNOTrainer(block, **kw, **self._opt_kw, **({} if self._step_lr else self._sch_kw))
            if self._step_lr:
                step, gamma = int(self._sch_kw["step_size"]), float(self._sch_kw["gamma"])
                tr.lr_factor = lambda: gamma ** (self.current_epoch // step)      # torch.optim.lr_scheduler.StepLR, per epoch
        return self._trainer


class EpochEndMixin(OptimizerMixin):
    """... and ``on_train_epoch_end``, for the routines whose caller counts the epochs (the Markov routine is told the epoch by
    every ``training_step(batch, epoch=...)`` and has no such hook)."""

    def on_train_epoch_end(self):
        self.current_epoch += 1
