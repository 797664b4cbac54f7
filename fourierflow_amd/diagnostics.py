"""What the reference computes from a trained model's test predictions for the paper's spectrum figure: the isotropic
kinetic-energy spectrum of velocity images (commands/plot.py:256-306, which reads the `preds.nc` that
routines/grid_2d_markov.py:427-476 writes) and the file itself -- written as the ``.npz`` sibling of the path, as
builders/kolmogorov.py reads ``.npz`` beside the ``.nc`` a config names.

    energy_spectrum(vx, vy)                      [..., m, m] device tensors -> [..., m/2+1], one ffno_energy_spectrum launch
    write_predictions(path, parts, times, ...)   the test batches' exported arrays -> one file for the whole split

The definition of the spectrum is this project's own (include/ffno.h): integer shells of unit width around |k| = s, Hermitian
weights for the half spectrum, E[s] summing to the mean of (u^2 + v^2) / 2 when the corner shells are added back.
"""
from __future__ import annotations

import os
from typing import Dict, Sequence

import numpy as np
import torch

from . import _capi, _lib
from .builders.kolmogorov import npz_path
from ._lib import ptr as _p

PRED_KEYS = ("pred_vorticity", "pred_vx", "pred_vy", "pred_energy_spectrum")
MIN_SIZE, MAX_SIZE = 8, 256


def check_size(m: int, what: str = "the grid size") -> int:
    """The sizes ffno_energy_spectrum takes: multiples of 8 from 8 to 256."""
    if int(m) != m or m % 8 or not MIN_SIZE <= m <= MAX_SIZE:
        raise ValueError(f"{what} must be a multiple of 8 between {MIN_SIZE} and {MAX_SIZE}, the sizes ffno_energy_spectrum takes "
                         f"(an odd size has no Nyquist column), got {m}")
    return int(m)


def _spectrum_of_pair(both: torch.Tensor) -> torch.Tensor:
    """both [2, ..., m, m] contiguous float32 (vx, vy) -> [..., m/2+1]: one batched rfft2, one ffno_energy_spectrum launch."""
    m = both.shape[-1]
    lead = tuple(both.shape[1:-2])
    n_img = int(np.prod(lead)) if lead else 1
    E = torch.empty(*lead, m // 2 + 1, dtype=torch.float32, device=both.device)
    if n_img == 0:
        return E
    spec = torch.view_as_real(torch.fft.rfft2(both)).contiguous()      # [2, ..., m, m/2+1, 2], unnormalised
    _capi.check(_lib.get_lib().ffno_energy_spectrum(_p(spec[0]), _p(spec[1]), _p(E), n_img, m, _lib.current_stream(both.device)),
                "energy_spectrum")
    return E


@torch.no_grad()
def energy_spectrum(vx: torch.Tensor, vy: torch.Tensor) -> torch.Tensor:
    """Isotropic kinetic-energy spectrum of velocity images vx, vy [..., m, m] (any leading dimensions, device tensors) ->
    [..., m/2+1]: one batched rfft2 and one ffno_energy_spectrum launch.  For the DNS files beside a model's predictions, say."""
    _lib.require_device_tensor(vx, "vx")
    _lib.require_device_tensor(vy, "vy")
    if vx.shape != vy.shape or vx.dim() < 2 or vx.shape[-1] != vx.shape[-2]:
        raise ValueError(f"vx and vy must be two [..., m, m] tensors of one shape, got {tuple(vx.shape)} and {tuple(vy.shape)}")
    check_size(vx.shape[-1], "the image size")
    return _spectrum_of_pair(torch.stack([vx.float(), vy.float()]).contiguous())


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_predictions(path: str, parts: Sequence[Dict[str, torch.Tensor]], times=None, *, domain=((0.0, 2 * np.pi), (0.0, 2 * np.pi)),
                      step_size: float = 1.0) -> str:
    """Write the exported arrays of the test batches `parts` (each the `pred_*` entries of Grid2DMarkovExperiment.test_step,
    time-major) as ONE file, the ``.npz`` sibling of `path` (``preds.nc`` -> ``preds.npz``; parent directories are created), and
    return its name.  The file holds, in the reference's layout (routines/grid_2d_markov.py:462-476):

        vorticity, vx, vy   [sample, x, y, time] float32, the batches concatenated along `sample`
        time                `times` (the batch's times[-n_steps:]) where given, else step_size * (1 .. n_steps)
        x, y                cell centres low + (i + 0.5) * length / pred_size, the reference's out_grid.axes()
        energy_spectrum     [sample, time, k], k = 0 .. pred_size / 2
    """
    if not parts:
        raise ValueError("write_predictions got no batch: nothing to write")
    missing = [k for k in PRED_KEYS if any(k not in p for p in parts)]
    if missing:
        raise ValueError(f"every part needs {', '.join(PRED_KEYS)} (the routine returns them when it has a pred_path); "
                         f"missing: {', '.join(missing)}")
    out = {}
    for key, name in zip(PRED_KEYS[:3], ("vorticity", "vx", "vy")):      # [n_steps, B, m, m] -> [B, m, m, n_steps]
        out[name] = np.concatenate([np.ascontiguousarray(np.transpose(_host(p[key]), (1, 2, 3, 0))) for p in parts]).astype(np.float32)
    out["energy_spectrum"] = np.concatenate([np.transpose(_host(p[PRED_KEYS[3]]), (1, 0, 2)) for p in parts]).astype(np.float32)
    n, m, _, n_steps = out["vorticity"].shape
    if times is None:
        out["time"] = float(step_size) * np.arange(1, n_steps + 1, dtype=np.float64)
    else:
        out["time"] = _host(times).reshape(-1)
        if out["time"].shape[0] != n_steps:
            raise ValueError(f"times holds {out['time'].shape[0]} entries, the predictions {n_steps} steps")
    for name, (low, high) in zip(("x", "y"), domain):
        out[name] = float(low) + (np.arange(m) + 0.5) * (float(high) - float(low)) / m
    out["k"] = np.arange(m // 2 + 1)
    target = npz_path(path)
    parent = os.path.dirname(os.path.abspath(target))
    os.makedirs(parent, exist_ok=True)
    with open(target, "wb") as f:      # (numpy.savez appends .npz to a NAME without it; a file object is written as it is)
        np.savez(f, **out)
    return target
