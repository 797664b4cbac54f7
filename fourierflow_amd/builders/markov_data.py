"""Training set of the Markov routine held on the device as whole trajectories -- the counterpart of the reference's
``DataLoader(shuffle=True, drop_last=False)`` over ``NavierStokesTrainingDataset`` (builders/ns_markov.py:36-41, 62-91) and over
``KolmogorovTorchDataset`` (builders/kolmogorov.py:111-139), without the expanded copies those datasets hold.

``data [n, M, N, T]`` (and ``f [n, M, N]`` or ``f [n, M, N, T]`` / ``mu [n]``) are uploaded once, in the layout of the files.  A pair id
``p = b P + j`` names trajectory ``b`` and input time ``t = t0 + j``:

    mode "ns_markov":   t0 = k, P = T - 2 k    x = data[b, ..., t], y = data[b, ..., t + k], dx = x - data[b, ..., t - k], dy = y - x
    mode "kolmogorov":  t0 = 0, P = T - k      x, y only

(k = 1 in ``ns_markov`` mode is the reference's dataset.)  A force with one map per snapshot, ``f [n, M, N, T]``, gives the pair
the map of its TARGET time, ``batch['f'] = f[b, ..., t + k]`` (NavierStokesTrainingDataset of builders/ns_contextual.py:63-66);
either way ``batch['f']`` is ``[B, M, N]``.  An epoch is a permutation of the ``n P`` ids, uploaded once as int32; each batch is
ONE ``ffno_markov_pairs_tf`` launch (``ffno_markov_pairs`` with the force's time axis) that reads its ids through a pointer into
that array, so a step costs no host work beyond the launch.

Order.  ``shuffle=False`` is the reference's ``(b t)`` order, p = 0, 1, 2, ...  ``shuffle=True`` draws ``torch.randperm(n P)``
once per epoch from a CPU ``torch.Generator`` seeded once with ``seed`` (consecutive draws: the same seed gives the same run).
``drop_last=False`` keeps the short last batch, as the reference does.

Data parallel -- the one deviation from the reference's DistributedSampler: every rank draws the SAME permutation (the seed is
not offset by the rank) and rank r takes batches r, r + world, ...; trailing batches that do not fill every rank are dropped,
so that all ranks take the same number of steps (the gradient all-reduce needs that).  The reference pads the index list by
repeating samples instead.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from .. import _capi, _lib

MODES = ("ns_markov", "kolmogorov")


def _tensor(a, what: str) -> torch.Tensor:
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = torch.as_tensor(a)
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {t.dtype}")
    return t


def _upload(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    """The set's own copy on `device` (on the emulator's CPU backend too: the caller's array is never aliased)."""
    out = t.contiguous().to(device)
    return out.clone() if out.data_ptr() == t.data_ptr() else out


class MarkovTrajectoryData:
    def __init__(self, data, f=None, mu=None, *, device, batch_size: int, mode: str = "ns_markov", k: int = 1, seed: int,
                 shuffle: bool = True, drop_last: bool = False, rank: int = 0, world: int = 1):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if batch_size < 1 or k < 1:
            raise ValueError(f"batch_size and k are at least 1, got {batch_size} and {k}")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} is not one of {world} ranks")
        self.device = torch.device(device)
        if _lib.is_test_backend() != (self.device.type == "cpu"):
            raise _lib.FFNOLibraryError(
                f"MarkovTrajectoryData on {self.device}: the HIP library draws batches from a set on an MI355X (cuda) device, "
                f"the emulator backend from CPU tensors; there is no CPU path")
        data = _tensor(data, "data")
        if data.dim() != 4:
            raise ValueError(f"data holds trajectories [n, M, N, T], got {tuple(data.shape)}")
        n, M, N, T = data.shape
        self.mode, self.k = mode, int(k)
        self.t0, self.P = (self.k, T - 2 * self.k) if mode == "ns_markov" else (0, T - self.k)
        if n < 1 or M < 1 or N < 1 or self.P < 1:
            need = 2 * self.k + 1 if mode == "ns_markov" else self.k + 1
            raise ValueError(f"mode {mode!r} with k={self.k} needs trajectories of at least {need} steps and one trajectory, "
                             f"got data {tuple(data.shape)}")
        if n * self.P > 2 ** 31 - 1:
            raise ValueError(f"{n} x {self.P} pairs do not fit the kernel's int32 ids")
        self.data = _upload(data, self.device)
        self.f = self.mu = None
        self.Tf = 0      # force maps per trajectory along f's last axis; 0: one map
        if f is not None:
            f = _tensor(f, "f")
            if tuple(f.shape) not in ((n, M, N), (n, M, N, T)):
                raise ValueError(f"f must be one force map per trajectory {(n, M, N)} or one per snapshot {(n, M, N, T)}, got "
                                 f"{tuple(f.shape)}")
            self.Tf = T if f.dim() == 4 else 0
            self.f = _upload(f, self.device)
        if mu is not None:
            mu = _tensor(mu, "mu")
            if tuple(mu.shape) != (n,):
                raise ValueError(f"mu must be one viscosity per trajectory {(n,)}, got {tuple(mu.shape)}")
            self.mu = _upload(mu, self.device)
        self.n, self.M, self.N, self.T = n, M, N, T
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        self.n_pairs = n * self.P
        total = self.n_pairs // self.batch_size if self.drop_last else -(-self.n_pairs // self.batch_size)
        self._batches = total // self.world * self.world      # the same number of batches on every rank
        if self._batches == 0:
            raise ValueError(f"{self.n_pairs} pairs give {total} batches of {self.batch_size}: not one for each of {self.world} ranks")
        self.gen = torch.Generator().manual_seed(int(seed))
        self._ids: Optional[torch.Tensor] = None

    def __len__(self) -> int:
        """Batches per epoch on this rank."""
        return self._batches // self.world

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        while True:
            yield from self.epoch()

    def _epoch_ids(self) -> torch.Tensor:
        if self.shuffle:
            self._ids = torch.randperm(self.n_pairs, generator=self.gen).to(torch.int32).to(self.device)
        elif self._ids is None:
            self._ids = torch.arange(self.n_pairs, dtype=torch.int32).to(self.device)
        return self._ids

    def epoch(self) -> Iterator[Dict[str, torch.Tensor]]:
        ids = self._epoch_ids()
        for j in range(self.rank, self._batches, self.world):
            lo = j * self.batch_size
            yield self.gather(ids, lo, min(self.batch_size, self.n_pairs - lo))

    def gather(self, ids: torch.Tensor, offset: int, B: int) -> Dict[str, torch.Tensor]:
        """The batch of the B pair ids at ids[offset:] (a device int32 array): one launch."""
        if ids.dtype != torch.int32 or ids.device != self.data.device or not ids.is_contiguous() or ids.dim() != 1:
            raise ValueError("ids must be a contiguous 1-D int32 tensor on the set's device")
        if B < 1 or offset < 0 or offset + B > ids.numel():
            raise ValueError(f"ids[{offset}:{offset + B}] is outside the {ids.numel()} ids given")
        dev, M, N = self.data.device, self.M, self.N

        def field():
            return torch.empty(B, M, N, 1, dtype=torch.float32, device=dev)

        b = dict(x=field(), y=field())
        if self.mode == "ns_markov":
            b.update(dx=field(), dy=field())
        if self.f is not None:
            b["f"] = torch.empty(B, M, N, dtype=torch.float32, device=dev)
        if self.mu is not None:
            b["mu"] = torch.empty(B, dtype=torch.float32, device=dev)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())

        rc = _lib.get_lib().ffno_markov_pairs_tf(p(self.data), ctypes.c_void_p(ids.data_ptr() + 4 * offset), p(b["x"]), p(b["y"]),
                                                 p(b.get("dx")), p(b.get("dy")), p(self.f), self.Tf, p(b.get("f")), p(self.mu),
                                                 p(b.get("mu")), self.n, M, N, self.T, self.t0, self.k, self.P, B,
                                                 _lib.current_stream(dev))
        _capi.check(rc, "markov_pairs")
        return b
