"""Batches without a builder: what the commands (fourierflow_amd/cli.py) read from ``--data FILE.npz`` / ``--init FILE.npz`` or draw
as synthetic fields of the routine's geometry."""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Iterator, List, Optional

import numpy as np
import torch

from ..routines import routine_kind
from .device_epochs import rank_share
from .markov_data import MarkovTrajectoryData


class Batches:
    """Batches of the routine's geometry: slices of an .npz file, or synthetic."""

    def __init__(self, routine, cfg, dev, data: Optional[Path], batch_size: Optional[int], grid: int, size: Optional[List[int]],
                 seed: int, rank: int = 0, world: int = 1):
        self.routine, self.dev, self.kind = routine, dev, routine_kind(routine)
        self.rank, self.world = rank, world      # data parallel: rank r takes every world-th batch of a file / its own stream
        seed = seed + 1000003 * rank
        self.B = batch_size or int(cfg.get("builder", {}).get("batch_size", 19))
        self.grid, self.size = grid, tuple(size) if size else None
        self.gen = torch.Generator().manual_seed(seed)
        self.arrays: Optional[Dict[str, np.ndarray]] = None
        if data is not None:
            with np.load(str(data)) as z:
                self.arrays = {k: z[k].astype(np.float32) for k in z.files}
            need = {"rollout": ("data",), "pointcloud": ("xy", "rr", "sigma")}.get(self.kind, ("x", "y"))
            if self.kind == "markov" and "data" in self.arrays:       # whole trajectories [n, M, N, T]: validation / test batches
                if self.arrays["data"].ndim != 4:
                    raise ValueError(f"{data}: a trajectory file holds data [n, M, N, T], got {self.arrays['data'].shape}")
                if len(self.arrays["data"]) < self.B:
                    raise ValueError(f"{data}: {len(self.arrays['data'])} trajectories do not fill one batch of {self.B}")
                need = ("data",)
            missing = [k for k in need if k not in self.arrays]
            if missing:
                raise ValueError(f"{data}: arrays {missing} missing (found {sorted(self.arrays)})")

    def _rand(self, *shape):
        return torch.randn(*shape, generator=self.gen).to(self.dev)

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        while True:
            yield from self.epoch()

    def epoch(self) -> Iterator[Dict[str, torch.Tensor]]:
        if self.arrays is not None:
            n = len(next(iter(self.arrays.values())))
            for j in rank_share(n // self.B, self.rank, self.world):
                i = j * self.B
                b = {k: torch.from_numpy(v[i:i + self.B]).to(self.dev) for k, v in self.arrays.items()}
                yield self._finish(b)
            return
        yield self._finish(self._synthetic())

    def _synthetic(self):
        B, G, r = self.B, self.grid, self.routine
        if self.kind == "rollout":
            return dict(data=self._rand(B, G, G, 10 + r.n_steps))
        if self.kind == "pointcloud":
            n = self.size[0] if self.size else 972
            return dict(xy=torch.rand(B, n, 2, generator=self.gen).to(self.dev), rr=self._rand(B, 42), sigma=self._rand(B, n, 1))
        if self.kind == "mesh":
            size = self.size or (G, G)
            cin = r.model.input_dim - len(size)
            return dict(x=self._rand(B, *size, cin), y=self._rand(B, *size, getattr(r.model, "output_dim", 1)))
        b = dict(x=self._rand(B, G, G, 1), y=self._rand(B, G, G, 1))
        if getattr(r, "append_force", False):
            b["f"] = self._rand(B, G, G)
        if getattr(r, "append_mu", False):
            b["mu"] = torch.rand(B, generator=self.gen).to(self.dev)
        return b

    def _finish(self, b):
        if self.kind == "rollout":      # the reference's forward() splits `data` and appends the positions (:38-50)
            d = b["data"]
            B, X, Y, _ = d.shape
            xx = torch.cat([d[..., :10], self.routine._positions(B, X, Y, d.device)], dim=-1)
            return dict(x=xx, y=d[..., 10:].contiguous())
        return b

    @property
    def trajectories(self) -> bool:
        return self.kind == "markov" and self.arrays is not None and "data" in self.arrays


def holds_trajectories(path: Path) -> bool:
    with np.load(str(path)) as z:
        return "data" in z.files


def trajectory_batches(routine, cfg, dev, path: Path, batch_size: Optional[int], mode: str, k: int, **kw):
    """The training set of a trajectory file on the device (builders/markov_data.py); `f` / `mu` go along when the routine
    appends them."""
    with np.load(str(path)) as z:
        arrays = {name: z[name].astype(np.float32) for name in ("data", "f", "mu") if name in z.files}
    missing = [name for name, on in (("f", routine.append_force), ("mu", routine.append_mu)) if on and name not in arrays]
    if missing:
        raise ValueError(f"{path}: arrays {missing} missing (found {sorted(arrays)})")
    return MarkovTrajectoryData(arrays["data"], arrays.get("f") if routine.append_force else None,
                                arrays.get("mu") if routine.append_mu else None, device=dev,
                                batch_size=batch_size or int(cfg.get("builder", {}).get("batch_size", 19)), mode=mode, k=k, **kw)


def initial_conditions(path: Path, routine) -> Dict[str, np.ndarray]:
    """x0 [n, M, N] [, f, mu] of an initial-condition file: `x0`, `vorticity` or `data`, as [n, M, N] or -- a trajectory array
    [n, M, N, T] -- its first time slice."""
    with np.load(str(path)) as z:
        name = next((k for k in ("x0", "vorticity", "data") if k in z.files), None)
        if name is None:
            raise ValueError(f"{path}: none of the arrays x0, vorticity, data (found {sorted(z.files)})")
        x0 = z[name].astype(np.float32)
        if x0.ndim == 4:
            x0 = x0[..., 0]
        if x0.ndim != 3:
            raise ValueError(f"{path}: {name} must be [n, M, N] or [n, M, N, T], got {list(z[name].shape)}")
        arrays = {"x0": np.ascontiguousarray(x0)}
        missing = [k for k, on in (("f", routine.append_force), ("mu", routine.append_mu)) if on and k not in z.files]
        if missing:
            raise ValueError(f"{path}: arrays {missing} missing (found {sorted(z.files)}): the config appends them to the input")
        for k, on in (("f", routine.append_force), ("mu", routine.append_mu)):
            if on:
                arrays[k] = z[k].astype(np.float32)
                if len(arrays[k]) != len(x0):
                    raise ValueError(f"{path}: {k} holds {len(arrays[k])} samples, {name} {len(x0)}")
    return arrays
