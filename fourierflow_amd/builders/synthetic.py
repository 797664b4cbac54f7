"""The 2-D Navier-Stokes data generator -- MI355X-native mirror of ``fourierflow.builders.synthetic`` (reference
builders/synthetic/ns_2d.py, random_fields.py): ``Force``, ``GaussianRF`` and ``solve_navier_stokes_2d`` with the reference's
signatures and return values.

The solver is the reference's pseudo-spectral Crank-Nicolson scheme (ns_2d.py:126-192) on ``torch.fft.rfft2`` half spectra.  Per
step: ``ffno_ns2d_derivs`` (the spectra of q, v, w_x, w_y from one read of w_h), one batched ``irfft2`` of the four,
``ffno_ns2d_advect`` (q w_x + v w_y), one ``rfft2``, ``ffno_ns2d_cn_update`` (dealias, force, update of w_h in place) -- three HIP
launches (csrc/ffno_ns2d.h) around two real rocFFT transforms, where the reference runs about forty element-wise launches around
five complex ones.  ``GaussianRF`` runs once per batch and stays plain torch, as in the reference.  HIP only: CPU tensors raise
(the tests route them through the emulator build of the same kernels).

``solve_navier_stokes_2d_varying_force`` is the reference's ``varying_force=True`` (ns_2d.py:118-119, 167-170, 188-195; an entry
of its own, because ``solve_navier_stokes_2d`` keeps its refusal of that argument): the random force with a phase that advances with time, a new field at
every step.  It is a sum of 3 cycles plane waves with fixed amplitudes and the common phase t_scaling t, so its half spectrum has
4 cycles non-zero bins per sample, fixed amplitudes rotated by e^{+-i phase}: ``ffno_ns2d_cn_update_harmonic`` computes them from the
amplitudes and (cos, sin) of the phase, and a step stays three launches around two transforms, with no force field, no force
transform and one half spectrum less to stream than a constant per-sample force.  ``ffno_ns2d_harmonic_force`` writes the field
itself, once per snapshot.
"""
from __future__ import annotations

import math
import os
from enum import Enum

import numpy as np
import torch

from .. import _capi, _lib
from .._lib import ptr as _p
from .npz_stream import NpzStream


class Force(str, Enum):
    li = 'li'
    random = 'random'
    none = 'none'
    kolmogorov = 'kolmogorov'


class GaussianRF:
    """Gaussian random field on the periodic unit square with covariance sigma^2 (-lap + tau^2)^(-alpha) (the 2-D case of the
    reference's random_fields.py): ``sample(n)`` -> [n, size, size], float32 on ``device``.

    Mode k of a sample is a complex standard normal times  size^2 sqrt(2) sigma (4 pi^2 |k|^2 + tau^2)^(-alpha / 2); the mean mode
    is left out and the field is the real part of the inverse transform.  sigma defaults to tau^(alpha - 1)."""

    def __init__(self, n_dims, size, alpha=2, tau=3, sigma=None, device=None):
        if n_dims != 2:
            raise NotImplementedError(f"GaussianRF: n_dims={n_dims}; only the 2-D field of `generate navier-stokes` is built")
        self.n_dims, self.size, self.device = 2, int(size), device
        if sigma is None:
            sigma = tau ** (alpha - 1.0)
        i = torch.arange(self.size, device=device)
        k = torch.where(i < self.size // 2, i, i - self.size).float()           # 0 .. size/2-1, -size/2 .. -1
        k2 = k[:, None] ** 2 + k[None, :] ** 2
        self.amplitude = self.size ** 2 * math.sqrt(2.0) * sigma * (4 * math.pi ** 2 * k2 + tau ** 2) ** (-0.5 * alpha)
        self.amplitude[0, 0] = 0.0

    def sample(self, n):
        # ONE normal draw of [n, size, size, 2], (real, imaginary) innermost: the order that ties the fields to the torch seed
        noise = torch.randn(n, self.size, self.size, 2, device=self.device)
        return torch.fft.ifft2(self.amplitude * torch.view_as_complex(noise)).real


def _unit_grid(N, device):
    """(X, Y), each [N, N]: the grid points i / N of the unit square, X along axis 0 and Y along axis 1."""
    g = torch.arange(N, dtype=torch.float32, device=device) / N
    return g[:, None].expand(N, N), g[None, :].expand(N, N)


def random_force_amplitudes(B, device, cycles, seed):
    """[cycles, 6, B]: the uniform amplitudes of the random force, from a generator on ``device`` seeded with ``seed``, one draw
    of [B, 1, 1] per term in the order (p; x, y, x + y; sin, cos) -- the draws of the reference's get_random_force, so that a seed
    gives the same force (one draw of all of them would give other numbers on the CPU generator)."""
    gen = torch.Generator(device)
    gen.manual_seed(seed)
    draws = [torch.rand(B, 1, 1, generator=gen, device=device).reshape(B) for _ in range(6 * cycles)]
    return torch.stack(draws).reshape(cycles, 6, B)


def random_force(B, N, device, cycles, scaling, seed):
    """[B, N, N]: per sample, ``scaling`` times the sum over p = 1 .. cycles of sin and cos of 2 pi p x, 2 pi p y and
    2 pi p (x + y), each with its own uniform amplitude from ``random_force_amplitudes``."""
    amplitudes = random_force_amplitudes(B, device, cycles, seed)
    X, Y = _unit_grid(N, device)
    f = torch.zeros(B, N, N, device=device)
    for p in range(1, cycles + 1):
        terms = [(phase, wave) for phase in (X, Y, X + Y) for wave in (torch.sin, torch.cos)]
        for i, (phase, wave) in enumerate(terms):
            f += amplitudes[p - 1, i][:, None, None] * wave(2 * math.pi * p * phase)
    return scaling * f


def _force_field(force, B, N, device, cycles, scaling, seed):
    """li: 0.1 (sin + cos)(2 pi (x + y)), [N, N]; kolmogorov: -4 cos(4 . 2 pi y), [N, N]; random: [B, N, N]; none: None."""
    if force == Force.none:
        return None
    if force == Force.random:
        return random_force(B, N, device, cycles, scaling, seed)
    X, Y = _unit_grid(N, device)
    if force == Force.kolmogorov:
        return -4 * torch.cos(8 * math.pi * Y)
    phase = 2 * math.pi * (X + Y)
    return 0.1 * (torch.sin(phase) + torch.cos(phase))


class SpectralStepper:
    """The state of one batch between steps: w_h, the half spectrum [B, N, N/2+1, 2] of the vorticity, advanced in place by
    ``step()`` (ns_2d.py:126-175): derivs -> irfft2 of the four spectra -> advect -> rfft2 -> cn_update.

    The force is None, one field [N, N], one per sample [B, N, N], or ``harmonic=(amplitudes [cycles, 6, B], scaling)``: the
    random force at the phase given to each ``step(phase)``, which the update computes in its bins; ``force_field(phase)`` is
    that force on the grid."""

    def __init__(self, w0, nu, f, delta_t, harmonic=None):
        self.lib = _lib.get_lib()
        self.B, self.N = int(w0.shape[0]), int(w0.shape[-1])
        dev = w0.device
        self.nu, self.delta_t = nu.contiguous(), float(delta_t)
        self.f_h = None if f is None else torch.view_as_real(torch.fft.rfft2(f.float())).contiguous()
        self.f_batched = int(self.f_h is not None and self.f_h.dim() == 4)
        self.amp = None
        if harmonic is not None:
            if f is not None:
                raise ValueError("SpectralStepper: a force field and a harmonic force at once")
            amplitudes, self.scaling = harmonic[0], float(harmonic[1])
            self.cycles = int(amplitudes.shape[0])
            if tuple(amplitudes.shape) != (self.cycles, 6, self.B) or not 1 <= self.cycles < self.N // 2:
                raise ValueError(f"harmonic force: amplitudes {tuple(amplitudes.shape)} for a batch of {self.B} on a grid of {self.N}; "
                                 f"expected [cycles, 6, {self.B}] with 1 <= cycles < {self.N // 2}")
            self.amp = amplitudes.to(device=dev, dtype=torch.float32).permute(2, 0, 1).contiguous()      # [B, cycles, 6]
        self.w_h = torch.view_as_real(torch.fft.rfft2(w0.contiguous())).contiguous()
        self.spec4 = torch.empty(4, self.B, self.N, self.N // 2 + 1, 2, dtype=torch.float32, device=dev)
        self.adv = torch.empty(self.B, self.N, self.N, dtype=torch.float32, device=dev)

    def step(self, phase=0.0):
        """One step; ``phase`` (a Python float) is the phase of the harmonic force in this step, read by no other force."""
        lib, B, N = self.lib, self.B, self.N
        st = _lib.current_stream(self.w_h.device)      # read per step: the transforms in between run on torch's current stream
        _capi.check(lib.ffno_ns2d_derivs(_p(self.w_h), _p(self.spec4), B, N, st), "ns2d_derivs")
        fields = torch.fft.irfft2(torch.view_as_complex(self.spec4), s=(N, N)).contiguous()      # q, v, w_x, w_y [4, B, N, N]
        _capi.check(lib.ffno_ns2d_advect(_p(fields), _p(self.adv), self.adv.numel(), st), "ns2d_advect")
        F_h = torch.view_as_real(torch.fft.rfft2(self.adv)).contiguous()
        if self.amp is not None:      # cos / sin in double on the host: two scalar arguments, no synchronisation, no extra launch
            _capi.check(lib.ffno_ns2d_cn_update_harmonic(_p(self.w_h), _p(F_h), _p(self.amp), _p(self.nu), self.delta_t, self.scaling,
                                                         math.cos(phase), math.sin(phase), self.cycles, B, N, st), "ns2d_cn_update_harmonic")
            return
        _capi.check(lib.ffno_ns2d_cn_update(_p(self.w_h), _p(F_h), _p(self.f_h), _p(self.nu), self.delta_t, self.f_batched, B, N, st),
                    "ns2d_cn_update")

    def force_field(self, phase):
        """[B, N, N]: the harmonic force at ``phase``."""
        f = torch.empty(self.B, self.N, self.N, dtype=torch.float32, device=self.w_h.device)
        _capi.check(self.lib.ffno_ns2d_harmonic_force(_p(self.amp), _p(f), self.scaling, math.cos(phase), math.sin(phase), self.cycles,
                                                      self.B, self.N, _lib.current_stream(f.device)), "ns2d_harmonic_force")
        return f

    def vorticity(self):
        return torch.fft.irfft2(torch.view_as_complex(self.w_h), s=(self.N, self.N))


def solve_navier_stokes_2d(w0, visc, T, delta_t, record_steps, cycles=None, scaling=None, t_scaling=None, force=Force.li,
                           varying_force=False):
    """Solve the 2-D Navier-Stokes equations in vorticity form with the Crank-Nicolson method (reference ns_2d.py:23-200).

    w0: initial vorticity [B, N, N] (float32, on the GPU; N a power of two, 8 ... 512); visc: viscosity, a float or a numpy
    array [B]; T: final time; delta_t: internal time step; record_steps: number of snapshots.
    Returns ``(sol, f)``: sol [B, N, N, record_steps] (numpy) and the force field (numpy; None for ``Force.none``).

    This entry solves with a force that is constant in time and keeps refusing ``varying_force=True``, as it always has
    (tests/test_ns2d_solver.py holds it to that): the time-varying force, whose second return value has another shape, is
    ``solve_navier_stokes_2d_varying_force`` with the same leading arguments.
    """
    seed = np.random.randint(1, 1000000000)      # drawn whatever the force is, like the reference (:46): same numpy stream
    force = Force(force)
    if varying_force:
        raise NotImplementedError("solve_navier_stokes_2d: varying_force (a new random force at every step, ns_2d.py:167-170) is "
                                  "solve_navier_stokes_2d_varying_force(w0, visc, T, delta_t, record_steps, cycles, scaling, "
                                  "t_scaling, force), which returns one force map per snapshot")
    return _solve(w0, visc, T, delta_t, record_steps, cycles, scaling, None, force, False, seed)


def solve_navier_stokes_2d_varying_force(w0, visc, T, delta_t, record_steps, cycles=None, scaling=None, t_scaling=None,
                                         force=Force.random):
    """The reference's ``solve_navier_stokes_2d(..., varying_force=True)`` (ns_2d.py:118-119, 167-170, 188-195), arguments as
    there: the random force of ``cycles`` and ``scaling`` with the phase ``t_scaling`` t, where t is the time before the step
    (:167-170, 178).  Returns ``(sol, fs)``, both [B, N, N, record_steps] (numpy): for every snapshot the force of the step that
    produced it (:188-189: not the force at the snapshot's time).  As in the reference, ``li`` and ``kolmogorov`` get the random
    force too; ``Force.none`` and a missing ``cycles``, ``scaling`` or ``t_scaling``, on which the reference fails at its first
    snapshot or step, are refused, and so is ``cycles >= N / 2``."""
    seed = np.random.randint(1, 1000000000)      # the reference's draw (:46)
    force = Force(force)
    if force == Force.none:
        raise ValueError("solve_navier_stokes_2d_varying_force: Force.none has no force to vary")
    if cycles is None or scaling is None or t_scaling is None:
        raise ValueError("solve_navier_stokes_2d_varying_force needs cycles, scaling and t_scaling")
    return _solve(w0, visc, T, delta_t, record_steps, cycles, scaling, t_scaling, force, True, seed)


def _solve(w0, visc, T, delta_t, record_steps, cycles, scaling, t_scaling, force, varying_force, seed):
    """The solver behind both entries; ``seed`` seeds the generator of the random force."""
    _lib.require_device_tensor(w0, "w0")
    if w0.dim() != 3 or w0.shape[1] != w0.shape[2]:
        raise ValueError(f"w0: expected [B, N, N], got {tuple(w0.shape)}")
    lib = _lib.get_lib()
    B, N = int(w0.shape[0]), int(w0.shape[-1])
    if not lib.ffno_ns2d_supported(N):
        raise ValueError(f"solve_navier_stokes_2d: grid size {N} is not a power of two in 8 ... 512 (ffno_ns2d_supported)")
    dev = w0.device
    steps = math.ceil(T / delta_t)
    record_time = math.floor(steps / record_steps)
    if record_time < 1:
        raise ValueError(f"{steps} solver steps cannot give {record_steps} snapshots")

    if isinstance(visc, np.ndarray):
        if visc.shape != (B,):
            raise ValueError(f"visc: expected a float or an array of shape ({B},), got {visc.shape}")
        nu = torch.from_numpy(np.ascontiguousarray(visc, dtype=np.float32)).to(dev)
    else:
        nu = torch.full((B,), float(visc), dtype=torch.float32, device=dev)

    if varying_force:
        if not 1 <= cycles < N // 2:
            raise ValueError(f"solve_navier_stokes_2d_varying_force: cycles={cycles} on a grid of {N}; 1 <= cycles < {N // 2}")
        f = None
        stepper = SpectralStepper(w0, nu, None, delta_t, harmonic=(random_force_amplitudes(B, dev, cycles, seed), scaling))
    else:
        f = _force_field(force, B, N, dev, cycles, scaling, seed)
        stepper = SpectralStepper(w0, nu, f, delta_t)
    snapshots, forces = [], []
    t = phase = 0.0      # t accumulates delta_t in Python floats, as the reference's does (:178)
    for _ in range(record_steps):      # a snapshot after every record_time steps; steps past the last snapshot change nothing
        for _ in range(record_time):
            phase = t_scaling * t if varying_force else 0.0
            stepper.step(phase)
            t += delta_t
        w = stepper.vorticity()
        if bool(torch.isnan(w).any()):
            raise ValueError(f"solve_navier_stokes_2d: NaN in snapshot {len(snapshots) + 1} of {record_steps}")
        snapshots.append(w)
        if varying_force:
            forces.append(stepper.force_field(phase))      # the force of the step that gave this snapshot
    if varying_force:
        f = torch.stack(forces, dim=-1)
    return torch.stack(snapshots, dim=-1).cpu().numpy(), (None if f is None else f.cpu().numpy())


def _target_force(f: np.ndarray):
    """f [n, M, N, T] -> [(n (T - 1)), M, N]: for every pair of ``_training_pairs``, in its order, the force map of the pair's
    target snapshot -- what NSContextualBuilder and ffno_markov_pairs_tf give a pair from a per-snapshot force."""
    n, M, N, T = f.shape
    return np.ascontiguousarray(np.moveaxis(f[..., 1:], -1, 1)).reshape(n * (T - 1), M, N)


def _training_pairs(u: np.ndarray):
    """u [n, M, N, T] -> x, y [(n (T - 1)), M, N, 1]: every snapshot with its successor, sample-major -- the (b t) order in which
    the reference's NavierStokesTrainingDataset enumerates its pairs (builders/ns_contextual.py:57-72 with k = 1)."""
    n, M, N, T = u.shape
    x = np.ascontiguousarray(np.moveaxis(u[..., :-1], -1, 1)).reshape(n * (T - 1), M, N, 1)
    y = np.ascontiguousarray(np.moveaxis(u[..., 1:], -1, 1)).reshape(n * (T - 1), M, N, 1)
    return x, y


def generate_navier_stokes(path: str, device, *, n_train: int, n_valid: int, n_test: int, s: int, t: float, steps: int, mu: float,
                           mu_min: float, mu_max: float, seed: int, delta: float, batch_size: int, force: Force, cycles: int,
                           scaling: float, ssr: int, train_trajectories: bool, t_scaling: float = 0.2,
                           varying_force: bool = False) -> dict:
    """The files of `generate navier-stokes` (fourierflow_amd/cli.py: the options are the command's): PATH.train.npz, PATH.valid.npz
    and PATH.test.npz, each solved `batch_size` trajectories at a time, with a shorter last batch where that does not divide the
    split, and written batch by batch.  `seed` seeds torch (initial vorticity) and, plus 1234, numpy (viscosity, force); the
    order of the draws below is what a seeded run reproduces.  With `varying_force` (the random force only) `f` holds one map per
    snapshot, [n, M, N, steps] beside `data`, and in the pair form of the training file the map of each pair's target.  Returns
    the command's summary."""
    if varying_force and force != Force.random:
        raise ValueError("generate_navier_stokes: varying_force goes with the random force")
    torch.manual_seed(seed)
    np.random.seed(seed + 1234)
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    field = GaussianRF(2, s, alpha=2.5, tau=7, device=device)
    n_solver = math.ceil(t / delta)
    times = (np.arange(1, steps + 1) * (n_solver // steps) * delta).astype(np.float32)
    vary_mu, pairs = mu_min != mu_max, steps - 1
    written = {}
    for split, n in (("train", n_train), ("valid", n_valid), ("test", n_test)):
        if n <= 0:
            continue
        as_pairs = split == "train" and not train_trajectories
        rows_per_sample = pairs if as_pairs else 1      # the per-sample f and mu are repeated for every pair
        sink = NpzStream(f"{path}.{split}.npz", n * rows_per_sample)
        done = 0
        while done < n:
            b = min(batch_size, n - done)
            # per batch, in this order: the initial vorticity from torch's generator; the viscosities, then (inside the solver)
            # the seed of the random force from numpy's
            with torch.no_grad():
                w0 = field.sample(b)
            nu = mu_min + (mu_max - mu_min) * np.random.rand(b) if vary_mu else mu
            if varying_force:
                sol, f = solve_navier_stokes_2d_varying_force(w0, nu, t, delta, steps, cycles, scaling, t_scaling, force)
            else:
                sol, f = solve_navier_stokes_2d(w0, nu, t, delta, steps, cycles, scaling, None, force, False)
            sol = sol[:, ::ssr, ::ssr]
            row = done * rows_per_sample
            if as_pairs:
                x, y = _training_pairs(sol)
                sink.put("x", row, x)
                sink.put("y", row, y)
            else:
                sink.put("data", row, sol)
                sink.put("times", row, np.tile(times, (b, 1)))
            if varying_force:
                sink.put("f", row, _target_force(f[:, ::ssr, ::ssr]) if as_pairs else f[:, ::ssr, ::ssr])
            elif force == Force.random:
                sink.put("f", row, np.repeat(f[:, ::ssr, ::ssr], rows_per_sample, axis=0))
            if vary_mu:
                sink.put("mu", row, np.repeat(nu, rows_per_sample))
            done += b
        written[split] = dict(file=sink.out, trajectories=n, **sink.close())
    return dict(solver_steps=n_solver, delta=delta, grid=s, ssr=ssr, varying_force=bool(varying_force), t_scaling=t_scaling, **written)
