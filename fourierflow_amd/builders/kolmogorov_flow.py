"""The Kolmogorov-flow data generator -- MI355X-native counterpart of ``fourierflow generate kolmogorov`` (reference
builders/kolmogorov.py:328-428, commands/generate.py) for the files under the reference's ``data/kolmogorov``: a pseudo-spectral
2-D Navier-Stokes solver on the periodic square [0, len)^2 (len = 2 pi in all but the ``large_domain`` files) with Kolmogorov
forcing and linear drag, saved at several ``(size, k)`` reductions as the ``.npz`` files that ``KolmogorovBuilder`` reads.

jax-cfd is neither installed nor part of the reference checkout, so this is the same equation and the same scheme written from
the formulas, not a replay of jax-cfd: in vorticity form, on ``rfft2`` half spectra,

    psi_h = w_h / |k|^2,  v_x = i k_y psi_h,  v_y = -i k_x psi_h
    E(w_h) = -filt rfft2(v_x w_x + v_y w_y) + c w_h + f_h          filt: 9 (kx^2 + ky^2) <= N^2 in indices (circular 2/3 rule)
    L      = -nu |k|^2 - drag
    f      = -magnitude k_f cos(k_f y_j),  y_j = (j + 1/2) len / N   (the curl of magnitude sin(k_f y) x^, at the cell centres)

and one time step is the low-storage Carpenter-Kennedy RK4(5) for E with Crank-Nicolson for L (``crank_nicolson_rk4``): for
s = 0..4   h <- E(w_h) + beta_s h,   w_h <- (w_h + gamma_s dt h + mu_s L w_h) / (1 - mu_s L),   mu_s = dt (alpha_{s+1} - alpha_s) / 2.
A stage is ``ffno_kf2d_derivs`` -> one batched ``irfft2`` -> ``ffno_ns2d_advect`` -> one ``rfft2`` -> ``ffno_kf2d_stage``
(csrc/ffno_kf2d.h); outputs below the simulation size go through ``ffno_kf2d_downsample`` (the staggered-velocity reduction of
utils/array.py:50-80).  The random initial fields are this project's own: jax's PRNG is not reproduced.  HIP only: CPU tensors
raise (the tests route them through the emulator build of the same kernels).
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _capi, _lib
from .._lib import ptr as _p
from .kolmogorov import load_initial, npz_path
from .npz_stream import NpzStream

TWO_PI = 2.0 * math.pi
ALPHA = (0.0, 0.1496590219993, 0.3704009573644, 0.6222557631345, 0.9582821306748, 1.0)
BETA = (0.0, -0.4178904745, -1.192151694643, -1.697784692471, -1.514183444257)
GAMMA = (0.1496590219993, 0.3792103129999, 0.8229550293869, 0.6994504559488, 0.1530572479681)

STEP_FN = "jax_cfd.spectral.time_stepping.crank_nicolson_rk4"
EQUATION = "fourierflow.utils.equations.NavierStokes2D"
STABLE_TIME_STEP = "jax_cfd.base.equations.stable_time_step"
TURBULENCE_FORCING = "jax_cfd.base.forcings.simple_turbulence_forcing"


def stable_time_step(max_velocity: float, max_courant_number: float, viscosity: float, dx: float) -> float:
    """jax-cfd's ``stable_time_step``: the smaller of the advective limit courant dx / max_velocity and the diffusive limit
    dx^2 / (4 nu) -- the 2-D case of dx^2 / (nu 2^ndim)."""
    return min(max_courant_number * dx / max_velocity, dx * dx / (4.0 * viscosity))


def forcing_bin(N: int, length: float, wavenumber: float, magnitude: float) -> Tuple[int, float, float]:
    """(kf, re, im): the one non-zero bin (row 0, column kf) of the half spectrum of f(y_j) = -magnitude k cos(k y_j),
    y_j = (j + 1/2) length / N; kf = k length / (2 pi) must be a whole number.  (0, 0, 0) without forcing."""
    if not magnitude or not wavenumber:
        return 0, 0.0, 0.0
    kf = wavenumber * length / TWO_PI
    if abs(kf - round(kf)) > 1e-9 or not 1 <= round(kf) <= N // 2 - 1:
        raise ValueError(f"forcing wavenumber {wavenumber} on a domain of length {length}: bin {kf} is not a whole number in "
                         f"1 ... {N // 2 - 1}")
    kf = int(round(kf))
    a = -magnitude * wavenumber * (N * N / 2.0)
    return kf, a * math.cos(math.pi * kf / N), a * math.sin(math.pi * kf / N)


class KolmogorovStepper:
    """The state of one batch between steps: w_h, the half spectrum [B, N, N/2+1, 2] of the vorticity, advanced in place by
    ``step()``; ``vorticity()`` and ``downsample(m)`` are the fields a snapshot stores."""

    def __init__(self, w0, viscosity, drag, dt, forcing_wavenumber=0, forcing_magnitude=0.0, linear_coefficient=0.0,
                 length=TWO_PI):
        _lib.require_device_tensor(w0, "w0")
        if w0.dim() != 3 or w0.shape[1] != w0.shape[2]:
            raise ValueError(f"w0: expected [B, N, N], got {tuple(w0.shape)}")
        self.lib = _lib.get_lib()
        self.B, self.N = int(w0.shape[0]), int(w0.shape[-1])
        B, N = self.B, self.N
        if not self.lib.ffno_kf2d_supported(N):
            raise ValueError(f"KolmogorovStepper: grid size {N} is not a power of two in 16 ... 4096 (ffno_kf2d_supported)")
        self.viscosity, self.drag, self.dt, self.c = float(viscosity), float(drag), float(dt), float(linear_coefficient)
        self.length, self.k0 = float(length), TWO_PI / float(length)
        self.kf, self.f_re, self.f_im = forcing_bin(N, self.length, forcing_wavenumber, forcing_magnitude)
        dev = w0.device
        self.w_h = torch.view_as_real(torch.fft.rfft2(w0.float().contiguous())).contiguous()
        self.h = torch.empty_like(self.w_h)
        self.spec4 = torch.empty(4, B, N, N // 2 + 1, 2, dtype=torch.float32, device=dev)
        self.adv = torch.empty(B, N, N, dtype=torch.float32, device=dev)

    def _derivs(self, st):
        _capi.check(self.lib.ffno_kf2d_derivs(_p(self.w_h), _p(self.spec4), self.k0, self.B, self.N, st), "kf2d_derivs")

    def step(self):
        lib, B, N = self.lib, self.B, self.N
        st = _lib.current_stream(self.w_h.device)      # read per step: the transforms in between run on torch's current stream
        for s in range(5):
            self._derivs(st)
            # v_x, v_y, w_x, w_y, each N^2 times too large: the 1 / N^2 of the inverse transform would be a pass of its own over
            # the four fields; the stage multiplies the product's spectrum by N^-4 instead (exact: N is a power of two)
            fields = torch.fft.irfft2(torch.view_as_complex(self.spec4), s=(N, N), norm="forward").contiguous()
            _capi.check(lib.ffno_ns2d_advect(_p(fields), _p(self.adv), self.adv.numel(), st), "ns2d_advect")
            adv_h = torch.view_as_real(torch.fft.rfft2(self.adv)).contiguous()
            mu = 0.5 * self.dt * (ALPHA[s + 1] - ALPHA[s])
            _capi.check(lib.ffno_kf2d_stage(_p(self.w_h), _p(self.h), _p(adv_h), self.viscosity, self.drag, self.c, self.dt, BETA[s],
                                            GAMMA[s], mu, self.kf, self.f_re, self.f_im, self.k0, float(N) ** -4, int(s == 0), B, N, st),
                        "kf2d_stage")

    def vorticity(self):
        return torch.fft.irfft2(torch.view_as_complex(self.w_h), s=(self.N, self.N))

    def velocity(self):
        """[2, B, N, N]: v_x, v_y on the grid."""
        self._derivs(_lib.current_stream(self.w_h.device))
        return torch.fft.irfft2(torch.view_as_complex(self.spec4[:2]), s=(self.N, self.N)).contiguous()

    def downsample(self, m: int, velocity=None):
        """The vorticity [B, m, m] of the staggered velocity reduced to m x m (utils/array.py:50-80); m = N: the vorticity itself
        (builders/kolmogorov.py:412-418).  ``velocity``: what ``velocity()`` returned for this state, to share among sizes."""
        m = int(m)
        if m == self.N:
            return self.vorticity()
        if m < 1 or self.N % m:
            raise ValueError(f"downsample: size {m} does not divide the simulation size {self.N}")
        vel = self.velocity() if velocity is None else velocity
        out = torch.empty(self.B, m, m, dtype=torch.float32, device=vel.device)
        _capi.check(self.lib.ffno_kf2d_downsample(_p(vel), _p(out), self.B, self.N, m, self.length,
                                                  _lib.current_stream(vel.device)), "kf2d_downsample")
        return out


def _sample_seed(seed: int, index: int) -> int:
    """The generator seed of sample ``index``: (seed, index) mixed by numpy's SeedSequence, whose output is stable across numpy
    versions.  Mixed because torch's CPU generator keeps 32 bits of its seed: seed 2^32 + index would drop ``seed``."""
    return int(np.random.SeedSequence([int(seed), int(index)]).generate_state(1, np.uint32)[0])


def initial_vorticity(n, N, max_velocity, peak_wavenumber, seed, first_index=0, device=None, length=TWO_PI):
    """[n, N, N] float32 on ``device``: random initial vorticity fields of samples first_index ... first_index + n - 1.  Sample i
    is white noise from a CPU generator seeded from (seed, i), shaped in Fourier space by |k|^(5/2) exp(-(|k| / k_p)^2) -- an
    energy spectrum ~ k^4 exp(-2 (k / k_p)^2), which peaks at k_p -- with no mean, scaled so that the largest speed
    sqrt(v_x^2 + v_y^2) on the grid, of the velocity as the solver derives it, is ``max_velocity``.  Computed per sample in float64 on the CPU, so a sample depends neither on
    the batch it is drawn in nor on the device."""
    k0 = TWO_PI / float(length)
    i = torch.arange(N)
    kx = (k0 * torch.where(i < N // 2, i, i - N).double())[:, None]
    ky = (k0 * torch.arange(N // 2 + 1).double())[None, :]
    k2 = kx ** 2 + ky ** 2
    shape = k2 ** 1.25 * torch.exp(-k2 / float(peak_wavenumber) ** 2)
    inv = torch.where(k2 > 0, 1.0 / k2.clamp_min(1e-300), torch.zeros_like(k2))
    dx, dy = kx.clone(), ky.clone()      # the derivative factors of the solver: zero at an axis' Nyquist bin (ffno_kf2d_derivs)
    dx[N // 2, 0], dy[0, N // 2] = 0.0, 0.0
    out = torch.empty(n, N, N, dtype=torch.float32)
    for j in range(n):
        gen = torch.Generator("cpu")
        gen.manual_seed(_sample_seed(seed, first_index + j))
        w_h = torch.fft.rfft2(torch.randn(N, N, generator=gen, dtype=torch.float64)) * shape
        w = torch.fft.irfft2(w_h, s=(N, N))
        w_h = torch.fft.rfft2(w)                      # of the real field: what a solver started from w sees
        psi = w_h * inv
        vx = torch.fft.irfft2(1j * dy * psi, s=(N, N))
        vy = torch.fft.irfft2(-1j * dx * psi, s=(N, N))
        out[j] = (w * (float(max_velocity) / torch.sqrt(vx ** 2 + vy ** 2).max())).float()
    return out if device is None else out.to(device)


# ------------------------------------------------------------------------------------------------------------------
@dataclass
class KolmogorovPlan:
    """What one data-generation YAML asks for: sizes, time step and step counts.  Holds no array."""
    N: int
    length: float
    dt: float
    viscosity: float
    drag: float
    forcing_wavenumber: float
    forcing_magnitude: float
    linear_coefficient: float
    out_sizes: List[Tuple[int, int]]      # (size, k)
    n_trajectories: int
    max_velocity: float
    peak_wavenumber: float
    seed: int
    inner_steps: int
    outer_steps: int
    warmup_steps: int
    init_path: Optional[str] = None
    out_vorticity: bool = True            # false (the short_trajectories files: v_x and v_y only) plans, but is not generated
    files: Dict[Tuple[int, int], str] = field(default_factory=dict)      # (size, k) -> the .npz written

    @property
    def solver_steps(self) -> int:
        return (self.warmup_steps if self.warmup_steps > 0 else self.outer_steps) * self.inner_steps


def _not_built(what: str, why: str):
    return NotImplementedError(f"generate kolmogorov: {what} is not built: {why} (see DESIGN.md section 7)")


def _target(node: Any) -> str:
    return str(node.get("_target_", "")) if isinstance(node, dict) else ""


def _scalar(v: Any) -> Any:
    from ..config import _resolve_scalar
    return _resolve_scalar(v)


def _deref(cfg: Dict[str, Any], v: Any) -> Any:
    """A whole-value ``${name}`` reference to a top-level key of the file (``${sim_grid}``, ``${domain}``, ``${time_step}``)."""
    while isinstance(v, str) and v.startswith("${") and v.endswith("}") and ":" not in v:
        v = cfg[v[2:-1].strip()]
    return v


def plan_kolmogorov(cfg: Dict[str, Any], config_path: str) -> KolmogorovPlan:
    """The plan of a loaded data-generation YAML (``config.load_config``) whose output files go beside ``config_path``.  Settings
    are read by name; nothing of jax-cfd is imported.  Raises NotImplementedError, naming the reason, for what is not built (``out_vorticity: false`` plans and is refused by
    ``generate_kolmogorov``)."""
    grid = _deref(cfg, cfg["sim_grid"])
    shape = [int(s) for s in _deref(cfg, grid["shape"])]
    if len(shape) != 2:
        raise _not_built(f"a {len(shape)}-dimensional grid {shape}", "the solver is the 2-D vorticity form")
    method = cfg.get("method")
    step_fn = _deref(cfg, cfg.get("step_fn"))
    equation = _deref(cfg, step_fn.get("equation")) if isinstance(step_fn, dict) else None
    down = _scalar(cfg.get("downsample_fn"))
    down = getattr(down, "name", down)
    if method == "projection" or "semi_implicit_navier_stokes" in _target(step_fn) or str(down).endswith("downsample_velocity"):
        raise _not_built(f"method: {method} (step_fn {_target(step_fn) or step_fn}, downsample_fn {down})",
                         "jax-cfd's finite-volume projection solver")
    if _target(step_fn) != STEP_FN or _target(equation) != EQUATION:
        raise _not_built(f"step_fn {_target(step_fn)!r} with equation {_target(equation)!r}",
                         f"the one solver is {STEP_FN} on {EQUATION}")
    if shape[0] != shape[1]:
        raise ValueError(f"sim_grid.shape {shape}: the grid is square")
    N = shape[0]
    domain = [[float(_scalar(e)) for e in side] for side in _deref(cfg, grid["domain"])]
    if any(lo != 0.0 for lo, _ in domain) or domain[0][1] != domain[1][1] or not domain[0][1] > 0:
        raise ValueError(f"sim_grid.domain {domain}: expected the square [0, len]^2")
    length = domain[0][1]
    viscosity = float(equation["viscosity"])
    if not equation.get("smooth", True):
        raise ValueError("step_fn.equation.smooth: false -- the advection term is always dealiased here")
    forcing = _deref(cfg, equation.get("forcing_fn"))
    kf, mag, c = 0.0, 0.0, 0.0
    if forcing is not None:
        name = _target(forcing)
        if name == "functools.partial":
            ref = _scalar(forcing["_args_"][0])
            name = getattr(ref, "name", str(ref))
        if name != TURBULENCE_FORCING:
            raise ValueError(f"step_fn.equation.forcing_fn {name!r}: the forcing is {TURBULENCE_FORCING}")
        mag, kf = float(forcing.get("constant_magnitude", 0.0)), float(forcing.get("constant_wavenumber", 0.0))
        c = float(forcing.get("linear_coefficient", 0.0))
    ts = _deref(cfg, step_fn.get("time_step", cfg.get("time_step")))
    if isinstance(ts, dict):
        if _target(ts) != STABLE_TIME_STEP:
            raise ValueError(f"time_step {_target(ts)!r}: a number or {STABLE_TIME_STEP}")
        dt = stable_time_step(float(ts["max_velocity"]), float(ts["max_courant_number"]), float(ts["viscosity"]), length / N)
    else:
        dt = float(ts)
    out_sizes = [(int(o["size"]), int(o.get("k", 1))) for o in cfg["out_sizes"]]
    for size, k in out_sizes:
        if size < 1 or N % size or k < 1:
            raise ValueError(f"out_sizes entry size={size}, k={k}: size divides the simulation size {N} and k is at least 1")
    plan = KolmogorovPlan(
        N=N, length=length, dt=dt, viscosity=viscosity, drag=float(equation.get("drag", 0.0)), forcing_wavenumber=kf,
        forcing_magnitude=mag, linear_coefficient=c, out_sizes=out_sizes, n_trajectories=int(cfg["n_trajectories"]),
        max_velocity=float(cfg.get("max_velocity", 7.0)), peak_wavenumber=float(cfg.get("peak_wavenumber", 4.0)),
        seed=int(cfg.get("seed", 0)), inner_steps=int(cfg.get("inner_steps", 25)), outer_steps=int(cfg.get("outer_steps", 200)),
        warmup_steps=int(cfg.get("warmup_steps", 40)),
        init_path=str(_scalar(cfg["init_path"])) if cfg.get("init_path") else None,
        out_vorticity=bool(cfg.get("out_vorticity", True)))
    forcing_bin(N, length, kf, mag)      # refuses a forcing that is no whole bin of this grid
    if plan.warmup_steps <= 0 and plan.outer_steps <= 0:
        raise ValueError("warmup_steps and outer_steps are both 0: nothing to generate")
    stem = os.path.splitext(str(config_path))[0]
    trajectories = plan.warmup_steps <= 0
    plan.files = {(size, k): (f"{stem}_{size}_{k}.npz" if trajectories else f"{stem}_{size}.npz") for size, k in out_sizes}
    return plan


def _stepper(plan: KolmogorovPlan, w0) -> KolmogorovStepper:
    return KolmogorovStepper(w0, plan.viscosity, plan.drag, plan.dt, plan.forcing_wavenumber, plan.forcing_magnitude,
                             plan.linear_coefficient, plan.length)


def _outputs(stepper: KolmogorovStepper, sizes: Sequence[int]) -> Dict[int, np.ndarray]:
    vel = stepper.velocity() if any(m != stepper.N for m in sizes) else None
    return {m: stepper.downsample(m, vel).cpu().numpy() for m in sizes}


def generate_kolmogorov(plan: KolmogorovPlan, device, batch_size: int = 1) -> Dict[str, Dict[str, List[int]]]:
    """Run ``plan`` and write its files, ``batch_size`` trajectories at a time (builders/kolmogorov.py:328-405 for every batch):
    with warmup_steps > 0 advance warmup_steps x inner_steps steps and write the downsampled final fields, ``vorticity``
    [n, size, size]; otherwise take outer_steps snapshots inner_steps steps apart and write, per (size, k), every k-th starting
    at the k-th as ``vorticity`` [n, outer_steps // k, size, size] with ``time`` [outer_steps // k].  Initial fields: the file
    ``init_path`` names (its .npz sibling at the simulation size) or ``initial_vorticity``.  The files are written through the streamed
    .npz writer (builders/npz_stream.py).  Returns {file: {array: shape}}."""
    if not plan.out_vorticity:
        raise _not_built("out_vorticity: false", "the files hold the vorticity; velocity outputs (vx, vy) are not written")
    n, N = plan.n_trajectories, plan.N
    if not _lib.get_lib().ffno_kf2d_supported(N):
        raise ValueError(f"generate kolmogorov: grid size {N} is not a power of two in 16 ... 4096 (ffno_kf2d_supported)")
    w_init = None
    if plan.init_path:
        w_init = load_initial(plan.init_path)
        if w_init.shape[0] < n or w_init.shape[1:] != (N, N):
            raise ValueError(f"{npz_path(plan.init_path)} holds initial conditions {list(w_init.shape)}; the plan needs "
                             f"[{n}, {N}, {N}]")
    sizes = sorted({size for size, _ in plan.out_sizes})
    warmup = plan.warmup_steps > 0
    sinks = {key: NpzStream(path, n) for key, path in plan.files.items()}
    try:
        for done in range(0, n, batch_size):
            b = min(batch_size, n - done)
            if w_init is not None:
                w0 = torch.from_numpy(w_init[done:done + b]).to(device)
            else:
                w0 = initial_vorticity(b, N, plan.max_velocity, plan.peak_wavenumber, plan.seed, done, device, plan.length)
            stepper = _stepper(plan, w0)
            if warmup:
                for _ in range(plan.warmup_steps * plan.inner_steps):
                    stepper.step()
                outs = _outputs(stepper, sizes)
                for (size, k), sink in sinks.items():
                    sink.put("vorticity", done, outs[size])
            else:
                for t in range(1, plan.outer_steps + 1):
                    for _ in range(plan.inner_steps):
                        stepper.step()
                    due = [(key, sink) for key, sink in sinks.items() if t % key[1] == 0]
                    outs = _outputs(stepper, sorted({key[0] for key, _ in due}))
                    for (size, k), sink in due:
                        sink.array("vorticity", (plan.outer_steps // k, size, size))[done:done + b, t // k - 1] = outs[size]
            if not bool(torch.isfinite(stepper.w_h).all()):
                raise ValueError(f"generate kolmogorov: trajectories {done} ... {done + b - 1} left the finite range (time step "
                                 f"{plan.dt} too large for this flow?)")
    except BaseException:
        for sink in sinks.values():      # leave no scratch directory of a run that wrote no file
            sink.abort()
        raise
    written = {}
    for (size, k), sink in sinks.items():
        shapes = sink.close()
        if not warmup:
            T = plan.outer_steps // k
            shapes.update(_append_array(sink.out, "time", plan.dt * plan.inner_steps * k * np.arange(1, T + 1, dtype=np.float64)))
        written[sink.out] = shapes
    return written


def _append_array(path: str, name: str, a: np.ndarray) -> Dict[str, List[int]]:
    import io
    import zipfile
    buf = io.BytesIO()
    np.save(buf, a)
    with zipfile.ZipFile(path, "a", zipfile.ZIP_STORED, allowZip64=True) as z:
        z.writestr(name + ".npy", buf.getvalue())
    return {name: list(a.shape)}
