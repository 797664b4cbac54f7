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

Order, drop-last and data parallel: the schedule of ``DeviceEpochs`` (builders/device_epochs.py) over the ``n P`` pair ids;
``shuffle=False`` is the reference's ``(b t)`` order, p = 0, 1, 2, ...

Several resolutions -- ``MultiResolutionMarkovData``, the counterpart of ``DataLoader(shuffle=True, num_workers=W)`` over
``KolmogorovMultiTorchDataset`` (builders/kolmogorov.py:142-174).  That dataset opens one file per grid size, indexes every file with
the same ``(b, t)`` and moves on to the next file after every ``batch_size`` items it has served.  Under a DataLoader with W workers

    every worker copies the dataset, its counter at zero, at the start of every epoch;
    batch j goes to worker j % W, as that worker's (j // W)-th batch;
    the worker advances its own file index after every ``batch_size`` items, i.e. after every batch it serves;
    the one short batch is the epoch's last, so it never shifts a phase

so batch j of an epoch is drawn entirely from file ``(j // W) % len(paths)``, and every epoch starts again at file 0.  Here every
file's trajectories are uploaded once, an epoch is ONE permutation of the ``n (T - k)`` pair ids shared by all sizes (the schedule
of ``DeviceEpochs``), and batch i of this rank's epoch is one ``ffno_markov_pairs_tf`` launch in mode ``kolmogorov`` on the array of
set ``(i // max(1, W)) % len(paths)``: ``x`` and ``y`` only.  Two deviations:

    num_workers = 0   the reference loads in the main process with ONE dataset object, whose counter runs on across epochs (and a
                      short batch leaves it mid-batch: the next epoch's batches mix two sizes and fail to stack, so this only runs
                      when n (T - k) is a multiple of the batch size).  Here it behaves as W = 1: every epoch starts at set 0.
    data parallel     the set index follows the rank's OWN batch position i, not the global batch number j = rank + i world: all
                      ranks step the same size together (the gradient all-reduce sums like with like).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterator, Sequence

import torch

from .. import _capi, _lib
from .._lib import ptr as p
from .device_epochs import DeviceEpochs, tensor, upload

MODES = ("ns_markov", "kolmogorov")


class MarkovTrajectoryData(DeviceEpochs):
    def __init__(self, data, f=None, mu=None, *, device, batch_size: int, mode: str = "ns_markov", k: int = 1, seed: int,
                 shuffle: bool = True, drop_last: bool = False, rank: int = 0, world: int = 1):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if batch_size < 1 or k < 1:
            raise ValueError(f"batch_size and k are at least 1, got {batch_size} and {k}")
        super().__init__(device=device, batch_size=batch_size, seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank,
                         world=world)
        data = tensor(data, "data")
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
        self.data = upload(data, self.device)
        self.f = self.mu = None
        self.Tf = 0      # force maps per trajectory along f's last axis; 0: one map
        if f is not None:
            f = tensor(f, "f")
            if tuple(f.shape) not in ((n, M, N), (n, M, N, T)):
                raise ValueError(f"f must be one force map per trajectory {(n, M, N)} or one per snapshot {(n, M, N, T)}, got "
                                 f"{tuple(f.shape)}")
            self.Tf = T if f.dim() == 4 else 0
            self.f = upload(f, self.device)
        if mu is not None:
            mu = tensor(mu, "mu")
            if tuple(mu.shape) != (n,):
                raise ValueError(f"mu must be one viscosity per trajectory {(n,)}, got {tuple(mu.shape)}")
            self.mu = upload(mu, self.device)
        self.n, self.M, self.N, self.T = n, M, N, T
        self.n_pairs = n * self.P
        self._schedule(self.n_pairs, "pairs", self.data)

    def _gather(self, ids: ctypes.c_void_p, B: int) -> Dict[str, torch.Tensor]:
        """The batch of B pair ids: one launch."""
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

        rc = _lib.get_lib().ffno_markov_pairs_tf(p(self.data), ids, p(b["x"]), p(b["y"]), p(b.get("dx")), p(b.get("dy")),
                                                 p(self.f), self.Tf, p(b.get("f")), p(self.mu), p(b.get("mu")), self.n, M, N, self.T, self.t0, self.k, self.P, B,
                                                 _lib.current_stream(dev))
        _capi.check(rc, "markov_pairs")
        return b


class MultiResolutionMarkovData(DeviceEpochs):
    """``arrays``: one ``data [n, M_s, N_s, T]`` per grid size, all with the same n and T (the same pair ids name the same
    ``(b, t)`` in every one).  ``num_workers``: the W of the schedule above."""

    def __init__(self, arrays: Sequence, *, device, batch_size: int, k: int = 1, num_workers: int = 0, seed: int,
                 shuffle: bool = True, drop_last: bool = False, rank: int = 0, world: int = 1):
        if len(arrays) < 1:
            raise ValueError("MultiResolutionMarkovData needs the trajectories of at least one grid size, got none")
        if num_workers < 0:
            raise ValueError(f"num_workers is at least 0, got {num_workers}")
        super().__init__(device=device, batch_size=batch_size, seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank,
                         world=world)
        # each size as a single-size set of its own: its array, its checks and its launch (their own schedules are not used)
        self.sets = [MarkovTrajectoryData(a, device=device, batch_size=batch_size, mode="kolmogorov", k=k, seed=0, shuffle=False)
                     for a in arrays]
        first = self.sets[0]
        for i, s in enumerate(self.sets):
            if (s.n, s.T) != (first.n, first.T):
                raise ValueError(f"set {i} holds {s.n} trajectories of {s.T} snapshots, set 0 {first.n} of {first.T}: every "
                                 f"grid size is indexed with the same (trajectory, time) pairs")
        self.mode, self.k, self.n, self.T, self.P = "kolmogorov", first.k, first.n, first.T, first.P
        self.sizes = [(s.M, s.N) for s in self.sets]
        self.stride = max(1, int(num_workers))      # consecutive batches of one set
        self.n_pairs = first.n_pairs
        self._schedule(self.n_pairs, "pairs", first.data)

    def set_index(self, i: int) -> int:
        """The set that batch i of this rank's epoch is drawn from."""
        return (i // self.stride) % len(self.sets)

    def epoch(self) -> Iterator[Dict[str, torch.Tensor]]:
        ids = self._draw()
        for i, lo, B in self._slices():
            yield self.sets[self.set_index(i)].gather(ids, lo, B)

    def gather(self, ids: torch.Tensor, offset: int, B: int, set_index: int = 0) -> Dict[str, torch.Tensor]:
        """The batch of the B ids at ids[offset:] from set `set_index`: one launch."""
        return self.sets[set_index].gather(ids, offset, B)
