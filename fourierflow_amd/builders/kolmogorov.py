"""The reference's dataset builder of the Kolmogorov-flow experiments, torus_kochkov -- ``KolmogorovBuilder`` with
``KolmogorovTorchDataset`` and ``KolmogorovTrajectoryDataset`` (builders/kolmogorov.py:30-68, 111-139, 177-212) -- with the same
constructor keywords and the interface of builders/ns_contextual.py: ``train_data`` / ``valid_data`` / ``test_data`` return sets held
on the device whose batches are one launch each, ``inference_data(device)`` the test trajectories.

Files.  The reference opens netCDF files (``.nc``, HDF5 inside) with xarray; this project reads neither.  Every ``P.nc`` that a
config names is read from ``P.npz`` beside it, and a path that ends in ``.npz`` is taken as it is.  A trajectory file holds
``vorticity [n, T, X, Y]`` (the reference's own dimension order) or ``data [n, X, Y, T]`` (what ``generate navier-stokes
--train-trajectories`` writes) and optionally ``time [T]`` (or that generator's ``times [n, T]``, whose first row is taken), default
``arange(1, T + 1)``; an initial-condition file holds ``vorticity [n, X, Y]``.  The datasets are light objects that hold paths,
``k`` and ``end`` (``in_memory`` is accepted and ignored) and load on first use.

Semantics: those of the reference's datasets.

    train   KolmogorovTorchDataset: the pairs x = w[b, ..., t], y = w[b, ..., t + k] for t = 0 ... T - k - 1 (its ``vx`` / ``vy`` items
            are not read by the routine): ``MarkovTrajectoryData`` in mode ``kolmogorov``, one ``ffno_markov_pairs`` launch per
            batch, shuffled, short last batch kept
    train, several grid sizes   KolmogorovMultiTorchDataset(paths, k, batch_size) (:142-174), built here under the project's own
            name ``KolmogorovMultiResolutionDataset``: one trajectory file per size, all with the same n and T, every batch drawn
            from ONE of them in the order ``num_workers`` loader processes would serve them: ``MultiResolutionMarkovData``
            (builders/markov_data.py has the schedule and its two deviations).  A config selects it with the override
            ``builder.train_dataset._target_=fourierflow_amd.builders.KolmogorovMultiResolutionDataset``
    valid / test   KolmogorovTrajectoryDataset: with S = slice(None, end, k),
                data      = concat([initial condition, trajectory], time)[..., S]
                times     = concat([0.0], time)[S]
                corr_data = corr trajectory[..., S]              WITHOUT an initial condition in front
            ``DeviceSampleData`` in file order, short last batch kept, one ``ffno_sample_gather`` launch per batch whose source
            stride along time is k; the initial condition is joined to the trajectory once, at load

The indexing is the reference's and is kept as it is: column j + 1 of ``data`` is trajectory snapshot k (j + 1) - 1, column j of
``corr_data`` is snapshot k j of the corr trajectory -- one snapshot later than the ``data`` column it is correlated with.  (The
routine compares the last n_steps columns of each; nothing here "aligns" them.)

``inference_data()`` is the reference's: the joined test trajectories at every k-th time, ``end`` not applied (:60-68).

Not built, and refused by name: ``KolmogorovJAXDataset`` and ``KolmogorovJAXTrajectoryDataset`` (the feeds of the
``LearnedInterpolator`` routine, jax-cfd) -- and the NAME ``fourierflow.builders.KolmogorovMultiTorchDataset``, which is not mapped to
the class above yet.  ``batch_size`` is used, ``num_workers`` by the multi-resolution set alone; the other loader
keywords (``pin_memory``, ``loader_target``) are accepted and ignored.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from .device_epochs import tensor, upload
from .markov_data import MarkovTrajectoryData, MultiResolutionMarkovData
from .sample_data import DeviceSampleData, Field, broadcast


def npz_path(path: str) -> str:
    """The file read for a path of a config: ``P.npz`` for ``P.nc``, the path itself otherwise."""
    path = os.path.expandvars(str(path))
    return path[:-len(".nc")] + ".npz" if path.endswith(".nc") else path


def _expected(path: str, problem: str) -> str:
    """The one message of every file problem: what was found, what is expected and how to convert."""
    return (f"{problem}.  KolmogorovBuilder reads {npz_path(path)}"
            f"{' (netCDF is not read here: the .npz file beside the .nc file that the config names)' if str(path).endswith('.nc') else ''}"
            f": a trajectory file holds `vorticity` [n, T, X, Y] or `data` [n, X, Y, T] and optionally `time` [T]; an "
            f"initial-condition file holds `vorticity` [n, X, Y].  Convert a netCDF file where xarray is installed with "
            f"`ds = xarray.open_dataset(P + '.nc'); numpy.savez(P + '.npz', vorticity=ds.vorticity.transpose('sample', 'time', 'x', "
            f"'y').values, time=ds.time.values)` (an initial-condition file has no time axis), or write trajectories with `python -m "
            f"fourierflow_amd generate navier-stokes PREFIX --train-trajectories`")


def _open(path: str):
    file = npz_path(path)
    if not os.path.isfile(file):
        raise FileNotFoundError(_expected(path, f"dataset file not found: {file}"))
    return file, np.load(file)


def load_trajectories(path: str):
    """(w [n, X, Y, T] float32, time [T] float64) of a trajectory file."""
    file, z = _open(path)
    with z:
        if "vorticity" in z.files:
            w = z["vorticity"]
            if w.ndim != 4:
                raise ValueError(_expected(path, f"{file}: `vorticity` of a trajectory file is [n, T, X, Y], got {list(w.shape)}"))
            w = np.moveaxis(w, 1, -1)
        elif "data" in z.files:
            w = z["data"]
            if w.ndim != 4:
                raise ValueError(_expected(path, f"{file}: `data` is [n, X, Y, T], got {list(w.shape)}"))
        else:
            raise ValueError(_expected(path, f"{file}: no array `vorticity` or `data` (found {sorted(z.files)})"))
        T = w.shape[-1]
        if "time" in z.files:
            time = np.asarray(z["time"], np.float64).reshape(-1)
        elif "times" in z.files:
            time = np.asarray(z["times"], np.float64).reshape(-1, T)[0]
        else:
            time = np.arange(1, T + 1, dtype=np.float64)
        if time.shape != (T,):
            raise ValueError(_expected(path, f"{file}: `time` holds {time.size} entries for trajectories of {T} snapshots"))
    return np.ascontiguousarray(w, dtype=np.float32), time


def load_initial(path: str) -> np.ndarray:
    """w0 [n, X, Y] float32 of an initial-condition file."""
    file, z = _open(path)
    with z:
        if "vorticity" not in z.files:
            raise ValueError(_expected(path, f"{file}: no array `vorticity` (found {sorted(z.files)})"))
        w0 = z["vorticity"]
    if w0.ndim != 3:
        raise ValueError(_expected(path, f"{file}: `vorticity` of an initial-condition file is [n, X, Y], got {list(w0.shape)}"))
    return np.ascontiguousarray(w0, dtype=np.float32)


class KolmogorovTorchDataset:
    """Paths and k of the training pairs; ``arrays()`` loads the trajectories on first use."""

    def __init__(self, path, k, in_memory=False):
        self.path, self.k = str(path), int(k)
        if self.k < 1:
            raise ValueError(f"k (the snapshots between input and target) is at least 1, got {k}")
        self._w: Optional[np.ndarray] = None

    def arrays(self) -> np.ndarray:
        if self._w is None:
            self._w, _ = load_trajectories(self.path)
            if self._w.shape[-1] <= self.k:
                raise ValueError(f"{npz_path(self.path)}: trajectories of T = {self._w.shape[-1]} snapshots, a pair k = {self.k} "
                                 f"apart needs at least {self.k + 1}")
        return self._w

    def __len__(self) -> int:
        w = self.arrays()
        return w.shape[0] * (w.shape[-1] - self.k)


class KolmogorovMultiResolutionDataset:
    """Paths (one trajectory file per grid size), k and batch size of the training pairs of a multi-resolution run -- the
    reference's ``KolmogorovMultiTorchDataset(paths, k, batch_size)`` (:142-174) under this project's own name; ``arrays()`` loads
    every file on first use.  The reference indexes every file with the same ``(b, t)``, so the files agree in n and T; each file's
    grid may differ from the others'."""

    def __init__(self, paths, k, batch_size):
        self.paths = [str(p) for p in ([paths] if isinstance(paths, (str, os.PathLike)) else list(paths or []))]
        self.k, self.batch_size = int(k), int(batch_size)
        if len(self.paths) < 1:
            raise ValueError("KolmogorovMultiResolutionDataset: paths names at least one trajectory file, got 0")
        if self.k < 1:
            raise ValueError(f"k (the snapshots between input and target) is at least 1, got {k}")
        if self.batch_size < 1:
            raise ValueError(f"batch_size is at least 1, got {batch_size}")
        self._ws: Optional[List[np.ndarray]] = None

    def arrays(self) -> List[np.ndarray]:
        """w [n, X_s, Y_s, T] of every path, in the order of ``paths``."""
        if self._ws is None:
            ws = [load_trajectories(path)[0] for path in self.paths]
            files = [npz_path(path) for path in self.paths]
            n, T = ws[0].shape[0], ws[0].shape[-1]
            for file, w in zip(files[1:], ws[1:]):
                if (w.shape[0], w.shape[-1]) != (n, T):
                    raise ValueError(f"{file} holds n = {w.shape[0]} trajectories of T = {w.shape[-1]} snapshots, {files[0]} n = {n} "
                                     f"of T = {T}: the files of a multi-resolution set are indexed with the same (trajectory, time) "
                                     f"pairs and must agree in both")
            if T <= self.k:
                raise ValueError(f"{', '.join(files)}: trajectories of T = {T} snapshots, a pair k = {self.k} apart needs at least "
                                 f"{self.k + 1}")
            self._ws = ws
        return self._ws

    def __len__(self) -> int:
        w = self.arrays()[0]
        return w.shape[0] * (w.shape[-1] - self.k)


class KolmogorovTrajectoryDataset:
    """Paths, k and end of a validation / test set; ``arrays()`` loads and joins on first use."""

    def __init__(self, init_path, path, corr_path, k, end=None, in_memory=False):
        self.init_path, self.path, self.corr_path = str(init_path), str(path), str(corr_path)
        self.k, self.end = int(k), None if end is None else int(end)
        if self.k < 1:
            raise ValueError(f"k (the stride along time) is at least 1, got {k}")
        self._arrays: Optional[Dict[str, np.ndarray]] = None

    def arrays(self) -> Dict[str, np.ndarray]:
        """full [n, X, Y, 1 + T] (the initial condition in front), time [1 + T] (0.0 in front), corr [n, m, m, Tc]."""
        if self._arrays is None:
            w, time = load_trajectories(self.path)
            w0 = load_initial(self.init_path)
            corr, _ = load_trajectories(self.corr_path)
            if w0.shape != w.shape[:3]:
                raise ValueError(f"{npz_path(self.init_path)} holds initial conditions {list(w0.shape)}, {npz_path(self.path)} "
                                 f"trajectories {list(w.shape)}: [n, X, Y] and [n, X, Y, T] must agree")
            if len(corr) != len(w):
                raise ValueError(f"{npz_path(self.corr_path)} holds {len(corr)} trajectories, {npz_path(self.path)} {len(w)}")
            self._arrays = dict(full=np.concatenate([w0[..., None], w], axis=-1), time=np.concatenate([[0.0], time]), corr=corr)
        return self._arrays

    def columns(self, T: int) -> range:
        """The time indices slice(None, end, k) picks from an axis of length T."""
        return range(*slice(None, self.end, self.k).indices(T))

    def __len__(self) -> int:
        return len(self.arrays()["full"])


def _refuse(name: str, why: str):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"fourierflow.builders.{name} is not built: {why} (see DESIGN.md section 7)")
    return type(name, (), {"__init__": __init__, "__doc__": f"Not built: {why}."})


KolmogorovMultiTorchDataset = _refuse("KolmogorovMultiTorchDataset",
                                      "training that alternates between several resolutions runs under the name "
                                      "fourierflow_amd.builders.KolmogorovMultiResolutionDataset (override "
                                      "builder.train_dataset._target_ with it); this name is not mapped to it yet")
KolmogorovJAXDataset = _refuse("KolmogorovJAXDataset", "it feeds the LearnedInterpolator routine (jax-cfd), which is not built")
KolmogorovJAXTrajectoryDataset = _refuse("KolmogorovJAXTrajectoryDataset",
                                         "it feeds the LearnedInterpolator routine (jax-cfd), which is not built")


class KolmogorovBuilder:
    name = "kolmogorov"

    def __init__(self, train_dataset, valid_dataset, test_dataset, loader_target: str = "torch.utils.data.DataLoader", **kwargs):
        for what, ds, cls in (("train_dataset", train_dataset, (KolmogorovTorchDataset, KolmogorovMultiResolutionDataset)),
                              ("valid_dataset", valid_dataset, (KolmogorovTrajectoryDataset,)),
                              ("test_dataset", test_dataset, (KolmogorovTrajectoryDataset,))):
            if not isinstance(ds, cls):
                raise TypeError(f"KolmogorovBuilder: {what} must be a {' or a '.join(c.__name__ for c in cls)}, got "
                                f"{type(ds).__name__}")
        self.train_dataset, self.valid_dataset, self.test_dataset = train_dataset, valid_dataset, test_dataset
        self.kwargs = dict(kwargs)
        self.batch_size = int(self.kwargs.get("batch_size", 1))      # DataLoader's default
        self.num_workers = int(self.kwargs.get("num_workers", 0))    # (likewise; read by the multi-resolution schedule only)
        if isinstance(train_dataset, KolmogorovMultiResolutionDataset) and train_dataset.batch_size != self.batch_size:
            raise ValueError(f"KolmogorovBuilder: train_dataset.batch_size = {train_dataset.batch_size} but the builder's batch_size "
                             f"= {self.batch_size}: the dataset changes its grid size after every {train_dataset.batch_size} "
                             f"items, so a batch of {self.batch_size} would hold images of two sizes (set both to the same number)")

    def train_data(self, device, seed: int = 0, rank: int = 0, world: int = 1, shuffle: bool = True,
                   drop_last: bool = False) -> Union[MarkovTrajectoryData, MultiResolutionMarkovData]:
        """``train_dataloader()``: ``DataLoader(shuffle=True, drop_last=False)`` over the pairs -- of one file, or of one file per
        grid size in the order ``num_workers`` loader processes would serve them (builders/markov_data.py)."""
        ds = self.train_dataset
        if isinstance(ds, KolmogorovMultiResolutionDataset):
            return MultiResolutionMarkovData(ds.arrays(), device=device, batch_size=self.batch_size, k=ds.k,
                                             num_workers=self.num_workers, seed=seed, shuffle=shuffle, drop_last=drop_last,
                                             rank=rank, world=world)
        return MarkovTrajectoryData(ds.arrays(), device=device, batch_size=self.batch_size, mode="kolmogorov", k=ds.k, seed=seed,
                                    shuffle=shuffle, drop_last=drop_last, rank=rank, world=world)

    def _eval_data(self, ds: KolmogorovTrajectoryDataset, device) -> DeviceSampleData:
        a = ds.arrays()
        full, corr, k = a["full"], a["corr"], ds.k
        n, X, Y, T = full.shape
        _, m, m2, Tc = corr.shape
        L, Lc = len(ds.columns(T)), len(ds.columns(Tc))
        if L < 2 or Lc < 1:
            raise ValueError(f"{npz_path(ds.path)}: slice(None, {ds.end}, {k}) keeps {L} of {T} snapshots (initial condition "
                             f"included) and {Lc} of {Tc} of the corr trajectory: a rollout needs two and one")
        fields = [Field("data", full, (X, Y, L), X * Y, L, (X * Y * T, 0, T, k), (0, L, 1)),
                  Field("corr_data", corr, (m, m2, Lc), m * m2, Lc, (m * m2 * Tc, 0, Tc, k), (0, Lc, 1)),
                  broadcast("times", np.ascontiguousarray(a["time"][ds.columns(T)], dtype=np.float32))]
        return DeviceSampleData(fields, n, device=device, batch_size=self.batch_size, shuffle=False)

    def valid_data(self, device) -> DeviceSampleData:
        """``val_dataloader()``: file order, the short last batch kept, one rank."""
        return self._eval_data(self.valid_dataset, device)

    def test_data(self, device) -> DeviceSampleData:
        """``test_dataloader()``."""
        return self._eval_data(self.test_dataset, device)

    def inference_data(self, device) -> Dict[str, torch.Tensor]:
        """``{'data': ...}`` on `device`: the joined test trajectories at every k-th time (``end`` is not applied: :60-68)."""
        full = self.test_dataset.arrays()["full"]
        return {"data": upload(tensor(np.ascontiguousarray(full[..., ::self.test_dataset.k]), "data"), torch.device(device))}
