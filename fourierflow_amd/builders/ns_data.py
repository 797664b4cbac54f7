"""The reference's dataset builders of the torus_li experiments -- ``NSMarkovBuilder`` (builders/ns_markov.py:12-106) and
``NSZongyiBuilder`` (builders/ns_zongyi.py:12-86) -- over ``NavierStokes_V1e-5_N1200_T20.mat`` (``u [n, X, Y, T]``), with the same
constructor keywords and splits and the interface of builders/mesh_data.py: ``train_data`` / ``valid_data`` / ``test_data`` return
sets held on the device (``MarkovTrajectoryData``, ``DeviceSampleData``) whose batches are one launch each, and
``inference_data`` the trajectories the reference times its inference on.

``u`` is read as float32 and subsampled ``[:, ::ssr, ::ssr]`` once on the host; nothing else is expanded there: the Markov pairs
are drawn from whole trajectories (``ffno_markov_pairs``), the Zongyi windows ``u[..., :n_steps]`` / ``u[..., n_steps:2 n_steps]``
and the two position channels are strided fields of ``ffno_sample_gather`` over the single uploaded copy of ``u``.

Both builders have NO validation split of their own: ``valid_data`` and ``test_data`` are the last ``test_size`` trajectories,
and ``train_size + test_size > n`` makes the two ranges overlap without complaint, as in the reference.

Files: ``.mat`` (up to v7.2, ``scipy.io.loadmat``, key ``u``) or ``.npz`` with ``u`` or ``data`` -- what
``generate navier-stokes --train-trajectories`` writes.  ``batch_size`` is used; the other loader keywords are accepted and
ignored.
"""
from __future__ import annotations

import os
from typing import Dict

import numpy as np
import torch

from .device_epochs import tensor, upload
from .markov_data import MarkovTrajectoryData
from .sample_data import DeviceSampleData, Field, broadcast, rows


def _load_u(data_path: str) -> np.ndarray:
    """``u [n, X, Y, T]`` of the file, as stored."""
    path = os.path.expandvars(str(data_path))
    if not os.path.isfile(path):
        raise FileNotFoundError(f"dataset file not found: {path}")
    if path.endswith(".npz"):
        with np.load(path) as z:
            key = next((k for k in ("u", "data") if k in z.files), None)
            if key is None:
                raise ValueError(f"{path}: no array `u` or `data` [n, X, Y, T] (found {sorted(z.files)})")
            u = z[key]
    else:
        import scipy.io
        try:
            u = scipy.io.loadmat(path, variable_names=("u",))
        except NotImplementedError as e:      # scipy reads MATLAB files up to v7.2
            raise ValueError(f"{path} is a MATLAB v7.3 file, which is HDF5 and which scipy.io.loadmat does not read ({e}): convert it "
                             f"to an .npz file holding `u` [n, X, Y, T] first") from e
        if "u" not in u:
            raise ValueError(f"{path}: no variable `u` [n, X, Y, T] (found {sorted(k for k in u if not k.startswith('__'))})")
        u = u["u"]
    if u.ndim != 4:
        raise ValueError(f"{path}: expected u [n, X, Y, T], got {u.shape}")
    return u


class _NSBuilder:
    """The subsampled trajectories and the two row ranges; subclasses give `train_data` and `_eval_fields(u)`."""

    def __init__(self, data_path: str, train_size: int, test_size: int, ssr: int, min_steps: int, why: str, kwargs):
        self.data_path, self.ssr = str(data_path), int(ssr)
        if self.ssr < 1:
            raise ValueError(f"ssr (the sub-sampling rate) is at least 1, got {ssr}")
        raw = _load_u(self.data_path)
        self.u = np.ascontiguousarray(raw[:, ::self.ssr, ::self.ssr], dtype=np.float32)
        n, _, _, T = self.u.shape
        self.train_size, self.test_size = int(train_size), int(test_size)
        if not 1 <= self.train_size <= n or not 1 <= self.test_size <= n:
            raise ValueError(f"{data_path}: train_size = {train_size} and test_size = {test_size} must each be 1 ... {n}, the "
                             f"number of trajectories in the file")
        if T < min_steps:
            raise ValueError(f"{data_path}: trajectories of T = {T} steps, {why} needs at least {min_steps}")
        self.kwargs = dict(kwargs)
        self.batch_size = int(self.kwargs.get("batch_size", 1))      # DataLoader's default

    def _eval_data(self, device) -> DeviceSampleData:
        return DeviceSampleData(self._eval_fields(self.u[-self.test_size:]), self.test_size, device=device,
                                batch_size=self.batch_size, shuffle=False)

    def valid_data(self, device) -> DeviceSampleData:
        """``val_dataloader()``: the TEST trajectories (the reference has no other held-out split), file order, the short last
        batch kept, one rank."""
        return self._eval_data(device)

    def test_data(self, device) -> DeviceSampleData:
        """``test_dataloader()``."""
        return self._eval_data(device)

    def inference_data(self, device) -> Dict[str, torch.Tensor]:
        """``{'data': u[:512]}`` on `device`: the first min(512, n) trajectories of the file AS IT IS -- the reference does not
        apply ``ssr`` here (ns_markov.py:57-59, ns_zongyi.py:66-68), and neither does this."""
        u = self.u if self.ssr == 1 else _load_u(self.data_path)
        return {"data": upload(tensor(u[:512], "u"), torch.device(device))}


class NSMarkovBuilder(_NSBuilder):
    """Training batches ``x, y, dx, dy [B, X, Y, 1]``: the one-step pairs of ``u[:train_size]`` at input times 1 ... T - 2
    (NavierStokesTrainingDataset), drawn by ``MarkovTrajectoryData`` in mode ``ns_markov`` with k = 1.  Validation / test batches
    ``data [B, X, Y, T]``, ``times [B, T] = arange(0, 20)[:T]`` (NavierStokesDataset; float32 here)."""
    name = "ns_markov"

    def __init__(self, data_path: str, train_size: int, test_size: int, ssr: int, **kwargs):
        super().__init__(data_path, train_size, test_size, ssr, 3, "a pair with its dx (t - 1, t, t + 1)", kwargs)

    def train_data(self, device, seed: int = 0, rank: int = 0, world: int = 1, shuffle: bool = True,
                   drop_last: bool = False) -> MarkovTrajectoryData:
        """``train_dataloader()``: ``DataLoader(shuffle=True, drop_last=False)`` over the pairs."""
        return MarkovTrajectoryData(self.u[:self.train_size], device=device, batch_size=self.batch_size, mode="ns_markov", k=1,
                                    seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank, world=world)

    def _eval_fields(self, u):
        T = u.shape[-1]
        return [rows("data", u), broadcast("times", np.arange(0, 20, dtype=np.float32)[:T])]


class NSZongyiBuilder(_NSBuilder):
    """Batches ``x [B, X, Y, n_steps (+ 2)]`` (``u[..., :n_steps]`` and, with ``append_pos``, the two position channels
    ``linspace(0, 1, X)`` -- the X ticks on BOTH axes, as in the reference, hence square grids only), ``y [B, X, Y, n_steps]``
    (``u[..., n_steps:2 n_steps]``) and ``times [B, 10] = arange(10, 20)`` (float32 here).  Train: the first ``train_size``
    samples, shuffled; valid and test: the last ``test_size``.  The two windows are fields of ONE uploaded copy of the split's
    ``u``; the positions are one ``[X, Y, 2]`` array that every sample reads."""
    name = "ns_zongyi"

    def __init__(self, data_path: str, train_size: int, test_size: int, ssr: int, n_steps: int, append_pos: bool = True, **kwargs):
        self.n_steps, self.append_pos = int(n_steps), bool(append_pos)
        if self.n_steps < 1:
            raise ValueError(f"n_steps is at least 1, got {n_steps}")
        super().__init__(data_path, train_size, test_size, ssr, 2 * self.n_steps, f"n_steps = {self.n_steps} inputs and as many targets",
                         kwargs)
        _, X, Y, _ = self.u.shape
        if X != Y:
            raise ValueError(f"{data_path}: NSZongyiBuilder takes square grids only (both position channels are built from the X "
                             f"ticks, ns_zongyi.py:30-32), got {X} x {Y}" + (f" after ssr = {self.ssr}" if self.ssr > 1 else ""))
        ticks = torch.linspace(0, 1, X).numpy()      # torch's float32 ticks, the reference's (and the rollout routine's) own
        self.pos = np.ascontiguousarray(np.stack(np.broadcast_arrays(ticks[:, None], ticks[None, :]), axis=-1))      # [X, Y, 2]
        self.times = np.arange(10, 20, dtype=np.float32)

    def _eval_fields(self, u):
        _, X, Y, T = u.shape
        S, C = self.n_steps, self.n_steps + (2 if self.append_pos else 0)
        fields = [Field("x", u, (X, Y, C), X * Y, S, (X * Y * T, 0, T, 1), (0, C, 1)),
                  Field("y", u, (X, Y, S), X * Y, S, (X * Y * T, S, T, 1), (0, S, 1))]
        if self.append_pos:
            fields.append(Field("x", self.pos, (X, Y, C), X * Y, 2, (0, 0, 2, 1), (S, C, 1)))
        return fields + [broadcast("times", self.times)]

    def train_data(self, device, seed: int = 0, rank: int = 0, world: int = 1, shuffle: bool = True,
                   drop_last: bool = False) -> DeviceSampleData:
        """``train_dataloader()``: ``DataLoader(shuffle=True, drop_last=False)``."""
        return DeviceSampleData(self._eval_fields(self.u[:self.train_size]), self.train_size, device=device,
                                batch_size=self.batch_size, seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank, world=world)
