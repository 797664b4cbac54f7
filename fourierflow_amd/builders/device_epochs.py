"""The epoch schedule of a set held on the device -- what ``MarkovTrajectoryData`` (builders/markov_data.py) and
``DeviceSampleData`` (builders/sample_data.py) share: an epoch is a permutation of the set's ``count`` ids, uploaded once as
int32, and each batch is ONE launch that reads its ids through a pointer into that array.

Order.  ``shuffle=False`` is id order, 0, 1, 2, ... (``arange``, built once).  ``shuffle=True`` draws ``torch.randperm(count)``
once per epoch from a CPU ``torch.Generator`` seeded once with ``seed`` (consecutive draws: the same seed gives the same run).
``drop_last=False`` keeps the short last batch, as the reference's loaders do.

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

from .. import _lib


def tensor(a, what: str) -> torch.Tensor:
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float32)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = torch.as_tensor(a)
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {t.dtype}")
    return t


def upload(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    """The set's own copy on `device` (on the emulator's CPU backend too: the caller's array is never aliased)."""
    out = t.contiguous().to(device)
    return out.clone() if out.data_ptr() == t.data_ptr() else out


def rank_share(total: int, rank: int, world: int) -> range:
    """Of `total` batches, the ones rank `rank` of `world` takes: rank, rank + world, ... -- the same number on every rank."""
    return range(rank, total // world * world, world)


class DeviceEpochs:
    """Base of the device-resident sets.  A subclass checks and uploads its own arrays between ``__init__`` and ``_schedule``
    and implements ``_gather(ids: c_void_p, B)``, the single launch of a batch."""

    def __init__(self, *, device, batch_size: int, seed: int, shuffle: bool, drop_last: bool, rank: int, world: int):
        if batch_size < 1:
            raise ValueError(f"batch_size is at least 1, got {batch_size}")
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} is not one of {world} ranks")
        self.device = torch.device(device)
        if _lib.is_test_backend() != (self.device.type == "cpu"):
            raise _lib.FFNOLibraryError(
                f"{type(self).__name__} on {self.device}: the HIP library draws batches from a set on an MI355X (cuda) device, "
                f"the emulator backend from CPU tensors; there is no CPU path")
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        self.gen = torch.Generator().manual_seed(int(seed))
        self._ids: Optional[torch.Tensor] = None

    def _schedule(self, count: int, noun: str, home: torch.Tensor):
        """`count` ids (`noun`: what they name, for the message) of a set whose arrays live where `home` does (the device with
        its index: what the ids of `gather` are compared with)."""
        self.count, self.device = int(count), home.device
        total = self.count // self.batch_size if self.drop_last else -(-self.count // self.batch_size)
        self._mine = rank_share(total, self.rank, self.world)
        if not self._mine:
            raise ValueError(f"{self.count} {noun} give {total} batches of {self.batch_size}: not one for each of {self.world} "
                             f"ranks")

    def __len__(self) -> int:
        """Batches per epoch on this rank."""
        return len(self._mine)

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        while True:
            yield from self.epoch()

    def skip_epochs(self, n: int):
        """Advance the permutation stream past `n` epochs (a resumed run): the next epoch is the (n + 1)-th of a fresh set with
        the same seed.  An unshuffled set draws nothing."""
        for _ in range(n if self.shuffle else 0):
            torch.randperm(self.count, generator=self.gen)

    def _draw(self) -> torch.Tensor:
        """The ids of the next epoch on the device, in its order: one draw from the permutation stream when shuffled."""
        if self.shuffle:
            self._ids = torch.randperm(self.count, generator=self.gen).to(torch.int32).to(self.device)
        elif self._ids is None:
            self._ids = torch.arange(self.count, dtype=torch.int32).to(self.device)
        return self._ids

    def _slices(self) -> Iterator[tuple]:
        """(i, offset, B) of this rank's batches of an epoch: its i-th batch reads ids[offset:offset + B]."""
        for i, j in enumerate(self._mine):
            lo = j * self.batch_size
            yield i, lo, min(self.batch_size, self.count - lo)

    def epoch(self) -> Iterator[Dict[str, torch.Tensor]]:
        ids = self._draw()
        for _, lo, B in self._slices():
            yield self.gather(ids, lo, B)

    def gather(self, ids: torch.Tensor, offset: int, B: int) -> Dict[str, torch.Tensor]:
        """The batch of the B ids at ids[offset:] (a device int32 array): one launch."""
        if ids.dtype != torch.int32 or ids.device != self.device or not ids.is_contiguous() or ids.dim() != 1:
            raise ValueError("ids must be a contiguous 1-D int32 tensor on the set's device")
        if B < 1 or offset < 0 or offset + B > ids.numel():
            raise ValueError(f"ids[{offset}:{offset + B}] is outside the {ids.numel()} ids given")
        return self._gather(ctypes.c_void_p(ids.data_ptr() + 4 * offset), B)
