"""The reference's dataset builders for the structured-mesh and point-cloud experiments -- ``StructuredMesh2DBuilder`` (airfoil,
pipe: builders/structured_mesh_2d.py), ``PlasticityBuilder`` (builders/plasticity.py) and ``ElasticityBuilder``
(builders/elasticity.py) -- with the same constructor keywords, files and splits.  Where the reference builds three
``DataLoader`` objects over host tensors, ``train_data`` / ``valid_data`` / ``test_data`` here return a ``DeviceSampleData``
(builders/sample_data.py): the split lives on the device and a batch is one ``ffno_sample_gather`` launch.

``batch_size`` is used; the other loader keywords (``num_workers``, ``pin_memory``, ...) are accepted and ignored.  ``.npy``
files are memory-mapped, so only the rows of the three splits (and of ``sigma`` only the selected channel) are read.
"""
from __future__ import annotations

import os
from typing import Dict, Tuple

import numpy as np

from .sample_data import DeviceSampleData, Field, rows

SPLITS = ("train", "valid", "test")


def _exists(path: str) -> str:
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f"dataset file not found: {path}")
    return str(path)


def _npy(path: str) -> np.ndarray:
    return np.load(_exists(path), mmap_mode="r")


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class _Builder:
    """Three row ranges of the files' sample axis and the loader keywords; subclasses give `_fields(lo, hi)`."""

    def __init__(self, n_file: int, bounds: Dict[str, Tuple[int, int]], what: str, kwargs):
        need = max(hi for _, hi in bounds.values())
        if min(lo for lo, _ in bounds.values()) < 0 or need > n_file:
            sizes = " + ".join(str(hi - lo) for lo, hi in (bounds[s] for s in SPLITS))
            raise ValueError(f"{what}: train_size + valid_size + test_size = {sizes} = "
                             f"{sum(hi - lo for lo, hi in bounds.values())} samples, the file holds {n_file}")
        self.bounds, self.kwargs = bounds, dict(kwargs)
        self.batch_size = int(self.kwargs.get("batch_size", 1))      # DataLoader's default

    def _data(self, split: str, device, **kw) -> DeviceSampleData:
        lo, hi = self.bounds[split]
        if hi <= lo:
            raise ValueError(f"the {split} split is empty ({split}_size = {hi - lo})")
        return DeviceSampleData(self._fields(lo, hi), hi - lo, device=device, batch_size=self.batch_size, **kw)

    def train_data(self, device, seed: int = 0, rank: int = 0, world: int = 1, shuffle: bool = True,
                   drop_last: bool = False) -> DeviceSampleData:
        """``train_dataloader()``: ``DataLoader(shuffle=True, drop_last=False)`` of the reference."""
        return self._data("train", device, seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank, world=world)

    def valid_data(self, device) -> DeviceSampleData:
        """``val_dataloader()``: file order, the short last batch kept, one rank."""
        return self._data("valid", device, shuffle=False)

    def test_data(self, device) -> DeviceSampleData:
        """``test_dataloader()``."""
        return self._data("test", device, shuffle=False)


class StructuredMesh2DBuilder(_Builder):
    """Batches ``x [B, X, Y, 2]`` (the two coordinate files interleaved in the copy: the reference's ``torch.stack([x1, x2], -1)``)
    and ``y [B, X, Y, 1]`` (channel ``output_dim`` of ``sigma [n, C, X, Y]``; the reference's ``[B, X, Y]`` with the channel axis
    the routine takes).  Split (structured_mesh_2d.py:40-46): train ``[:i]``, TEST ``[i:i + test]``, valid after that -- the test
    set of the geo-FNO paper."""
    name = "structured_mesh_2d"

    def __init__(self, x1_path: str, x2_path: str, sigma_path: str, output_dim: int, train_size: int, valid_size: int,
                 test_size: int, **kwargs):
        self.x1, self.x2, self.sigma = _npy(x1_path), _npy(x2_path), _npy(sigma_path)
        self.output_dim = int(output_dim)
        if self.x1.ndim != 3 or self.x1.shape != self.x2.shape or self.sigma.ndim != 4 or \
                (self.sigma.shape[0],) + self.sigma.shape[2:] != self.x1.shape or not 0 <= self.output_dim < self.sigma.shape[1]:
            raise ValueError(f"expected x1, x2 [n, X, Y] and sigma [n, C, X, Y] with C > output_dim = {output_dim}, got "
                             f"{self.x1.shape}, {self.x2.shape}, {self.sigma.shape}")
        i, j, k = train_size, train_size + test_size, train_size + test_size + valid_size
        super().__init__(len(self.x1), dict(train=(0, i), test=(i, j), valid=(j, k)), x1_path, kwargs)

    def _fields(self, lo, hi):
        _, X, Y = self.x1.shape
        x1, x2, y = _f32(self.x1[lo:hi]), _f32(self.x2[lo:hi]), _f32(self.sigma[lo:hi, self.output_dim])
        return [Field("x", x1, (X, Y, 2), X * Y, 1, (X * Y, 0, 1, 0), (0, 2, 0)),
                Field("x", x2, (X, Y, 2), X * Y, 1, (X * Y, 0, 1, 0), (1, 2, 0)),
                rows("y", y, (X, Y, 1))]


class PlasticityBuilder(_Builder):
    """Batches ``x [B, s1, s2, t, 1]`` (``input [n, s1]`` of the .mat file broadcast in the copy: the reference's
    ``repeat(x, 'b s1 -> b s1 s2 t 1')``, whose expanded copy is never made) and ``y [B, s1, s2, t, 4]`` (``output``).  Split
    (plasticity.py:35-41): train, valid, test in order."""
    name = "plasticity"

    def __init__(self, data_path: str, train_size: int, valid_size: int, test_size: int, s1: int, s2: int, t: int, **kwargs):
        import scipy.io
        data = scipy.io.loadmat(_exists(data_path), variable_names=("input", "output"))
        self.x, self.y = data["input"], data["output"]
        self.s1, self.s2, self.t = int(s1), int(s2), int(t)
        if self.x.shape[1:] != (self.s1,) or self.y.shape[:-1] != (len(self.x), self.s1, self.s2, self.t):
            raise ValueError(f"expected input [n, {s1}] and output [n, {s1}, {s2}, {t}, C], got {self.x.shape} and {self.y.shape}")
        i, j, k = train_size, train_size + valid_size, train_size + valid_size + test_size
        super().__init__(len(self.x), dict(train=(0, i), valid=(i, j), test=(j, k)), data_path, kwargs)

    def _fields(self, lo, hi):
        s1, inner = self.s1, self.s2 * self.t
        return [Field("x", _f32(self.x[lo:hi]), (s1, self.s2, self.t, 1), s1, inner, (s1, 0, 1, 0), (0, inner, 1)),
                rows("y", _f32(self.y[lo:hi]))]


class ElasticityBuilder(_Builder):
    """Batches ``xy [B, N, 2]``, ``rr [B, 42]``, ``sigma [B, N, 1]``.  The files keep the sample axis LAST (``xy [N, 2, n]``,
    ``sigma [N, n]``, ``rr [42, n]``); the reference permutes them at load (elasticity.py:23-36), and so does this builder, once per
    split on the host: sample-major rows are then copied with coalesced, 16-byte accesses where aligned, which reading from the
    files' layout (``src_sample = 1``: every value of a sample n floats from the next) cannot be; timed back to back the two do
    not differ measurably (profiles/sample_data_path.md).  Split (elasticity.py:38-49):
    train from the front, valid ``[-eval:-test]`` and test ``[-test:]`` from the END."""
    name = "elasticity"

    def __init__(self, sigma_path: str, xy_path: str, rr_path: str, train_size: int, valid_size: int, test_size: int, **kwargs):
        self.rr, self.sigma, self.xy = _npy(rr_path), _npy(sigma_path), _npy(xy_path)
        n = self.rr.shape[-1]
        if self.rr.ndim != 2 or self.sigma.ndim != 2 or self.xy.ndim != 3 or self.xy.shape != (self.sigma.shape[0], 2, n) or \
                self.sigma.shape[1] != n:
            raise ValueError(f"expected rr [R, n], sigma [N, n] and xy [N, 2, n], got {self.rr.shape}, {self.sigma.shape}, "
                             f"{self.xy.shape}")
        ev = valid_size + test_size
        super().__init__(n, dict(train=(0, train_size), valid=(n - ev, n - test_size), test=(n - test_size, n)), rr_path, kwargs)

    def _fields(self, lo, hi):
        N = self.sigma.shape[0]
        return [rows("xy", _f32(np.transpose(self.xy[..., lo:hi], (2, 0, 1)))),
                rows("rr", _f32(np.transpose(self.rr[:, lo:hi]))),
                rows("sigma", _f32(np.transpose(self.sigma[:, lo:hi])), (N, 1))]
