"""The reference's dataset builder of the contextual Navier-Stokes experiments, torus_vis and torus_vis_force --
``NSContextualBuilder`` (builders/ns_contextual.py:10-101) -- with the same constructor keywords ``data_path, ssr, k`` and the
interface of builders/ns_data.py: ``train_data`` / ``valid_data`` / ``test_data`` return sets held on the device whose batches
are one launch each.

Files.  The reference opens ONE HDF5 file with the groups ``train`` / ``valid`` / ``test``, each holding ``u``, ``f``, ``mu``;
this project does not read HDF5.  The three groups are three ``.npz`` files instead, ``P.train.npz``, ``P.valid.npz`` and
``P.test.npz`` -- what ``generate navier-stokes P --train-trajectories --force random --mu-min .. --mu-max ..`` writes -- each
holding ``data`` (or ``u``) ``[n, X, Y, T]``, ``f`` ``[n, X, Y]`` or ``[n, X, Y, T]`` and ``mu`` ``[n]``.  ``data_path`` names the
prefix ``P``, any one of the three files, or ``P.h5`` (the shipped configs' own name) beside which the three files lie.

Semantics: those of the reference's two datasets, applied to whatever resolution the files hold (``ssr`` strides both grid axes
once on the host at load; files that are sub-sampled already take ``builder.ssr=1``).

    train   NavierStokesTrainingDataset (:45-72): the pairs x = u[b, ..., t], y = u[b, ..., t + k] for t = 0 ... T - k - 1 with
            mu[b] and the force f[b] or -- a force per snapshot -- f[b, ..., t + k]: ``MarkovTrajectoryData`` in mode
            ``kolmogorov``, one ``ffno_markov_pairs_tf`` launch per batch, shuffled, short last batch kept
    valid / test   NavierStokesDataset (:75-101): data = u[b, ..., ::k], f[b] or f[b, ..., ::k], mu[b] and
            times = arange(0, 20, 0.1 k) (float32 here): ``DeviceSampleData`` in file order, short last batch kept, one
            ``ffno_sample_gather`` launch per batch whose source stride along time is k -- the full-rate ``u`` is uploaded once
            and no strided copy is made on the host

``f`` / ``mu`` go into the batches only where the routine appends them (``append_force`` / ``append_mu``, which ``--builder``
sets from the routine; both default to True).  ``batch_size`` is used; the other loader keywords are accepted and ignored.  The
reference gives this builder no ``inference_data()``, and neither does this.
"""
from __future__ import annotations

import os
from typing import Dict

import numpy as np

from .markov_data import MarkovTrajectoryData
from .sample_data import DeviceSampleData, Field, broadcast, rows

SPLITS = ("train", "valid", "test")


def _expected(prefix: str, problem: str) -> str:
    """The one message of every file problem: what was found, what is expected and the command that writes it."""
    names = ", ".join(f"{prefix}.{s}.npz" for s in SPLITS)
    return (f"{problem}.  NSContextualBuilder reads the three files {names} (the groups train / valid / test of the reference's HDF5 "
            f"file, which is not read here), each holding `data` or `u` [n, X, Y, T], `f` [n, X, Y] or [n, X, Y, T] and `mu` [n]; "
            f"`python -m fourierflow_amd generate navier-stokes {prefix} --train-trajectories --force random --mu-min LOW "
            f"--mu-max HIGH` writes them")


def split_files(data_path: str) -> Dict[str, str]:
    """{split: file} for a `data_path` that names the prefix P, one of P.{train,valid,test}.npz, or P.h5."""
    path = os.path.expandvars(str(data_path))
    prefix = path
    for s in SPLITS:
        if path.endswith(f".{s}.npz"):
            prefix = path[:-len(f".{s}.npz")]
    if path.endswith(".h5"):
        prefix = path[:-len(".h5")]
    files = {s: f"{prefix}.{s}.npz" for s in SPLITS}
    missing = [f for f in files.values() if not os.path.isfile(f)]
    if missing:
        what = f"{path} is an HDF5 file name and its .npz siblings are not there: " if path.endswith(".h5") else ""
        raise FileNotFoundError(_expected(prefix, f"{what}dataset file{'s' if len(missing) > 1 else ''} not found: {', '.join(missing)}"))
    for f in files.values():      # (the zip directory alone is read here)
        with np.load(f) as z:
            absent = [k for k, on in (("data` or `u", "data" in z.files or "u" in z.files), ("f", "f" in z.files),
                                      ("mu", "mu" in z.files)) if not on]
            if absent:
                raise ValueError(_expected(prefix, f"{f}: no array `{'`, `'.join(absent)}` (found {sorted(z.files)})"))
    return files


class NSContextualBuilder:
    name = "ns_contextual"

    def __init__(self, data_path: str, ssr: int, k: int, **kwargs):
        self.data_path, self.ssr, self.k = str(data_path), int(ssr), int(k)
        if self.ssr < 1 or self.k < 1:
            raise ValueError(f"ssr (the sub-sampling rate) and k (the steps between input and target) are at least 1, got {ssr} and {k}")
        self.files = split_files(self.data_path)
        self.kwargs = dict(kwargs)
        self.batch_size = int(self.kwargs.get("batch_size", 1))      # DataLoader's default
        self.append_force = self.append_mu = True
        self.times = np.arange(0, 20, 0.1 * self.k).astype(np.float32)
        self._arrays: Dict[str, Dict[str, np.ndarray]] = {}

    def arrays(self, split: str) -> Dict[str, np.ndarray]:
        """u [n, X, Y, T], f [n, X, Y(, T)] and mu [n] of a split, float32, the grid strided by ssr; read once."""
        if split not in self._arrays:
            path, s = self.files[split], self.ssr
            with np.load(path) as z:
                u, f, mu = z["data" if "data" in z.files else "u"], z["f"], z["mu"]
            if u.ndim != 4 or mu.shape != u.shape[:1] or f.shape not in (u.shape[:3], u.shape):
                raise ValueError(f"{path}: expected data [n, X, Y, T], f [n, X, Y] or [n, X, Y, T] and mu [n], got {u.shape}, "
                                 f"{f.shape} and {mu.shape}")
            if u.shape[-1] <= self.k:
                raise ValueError(f"{path}: trajectories of T = {u.shape[-1]} steps, a pair k = {self.k} steps apart needs at least "
                                 f"{self.k + 1}")
            self._arrays[split] = dict(u=np.ascontiguousarray(u[:, ::s, ::s], dtype=np.float32),
                                       f=np.ascontiguousarray(f[:, ::s, ::s], dtype=np.float32),
                                       mu=np.ascontiguousarray(mu, dtype=np.float32))
        return self._arrays[split]

    def train_data(self, device, seed: int = 0, rank: int = 0, world: int = 1, shuffle: bool = True,
                   drop_last: bool = False) -> MarkovTrajectoryData:
        """``train_dataloader()``: ``DataLoader(shuffle=True, drop_last=False)`` over the pairs."""
        a = self.arrays("train")
        return MarkovTrajectoryData(a["u"], a["f"] if self.append_force else None, a["mu"] if self.append_mu else None, device=device,
                                    batch_size=self.batch_size, mode="kolmogorov", k=self.k, seed=seed, shuffle=shuffle,
                                    drop_last=drop_last, rank=rank, world=world)

    def _eval_data(self, split: str, device) -> DeviceSampleData:
        a = self.arrays(split)
        u, f, k = a["u"], a["f"], self.k
        n, X, Y, T = u.shape
        L = -(-T // k)                                   # len(range(0, T, k)): the snapshots 0, k, 2 k, ...

        def every_kth(out, source):
            return Field(out, source, (X, Y, L), X * Y, L, (X * Y * T, 0, T, k), (0, L, 1))

        fields = [every_kth("data", u)]
        if self.append_force:
            fields.append(every_kth("f", f) if f.ndim == 4 else rows("f", f))
        if self.append_mu:
            fields.append(rows("mu", a["mu"]))
        fields.append(broadcast("times", self.times))
        return DeviceSampleData(fields, n, device=device, batch_size=self.batch_size, shuffle=False)

    def valid_data(self, device) -> DeviceSampleData:
        """``val_dataloader()``: the valid file, file order, the short last batch kept, one rank."""
        return self._eval_data("valid", device)

    def test_data(self, device) -> DeviceSampleData:
        """``test_dataloader()``: the test file."""
        return self._eval_data("test", device)
