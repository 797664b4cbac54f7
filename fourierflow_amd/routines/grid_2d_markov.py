"""Markov one-step training routine around the F-FNO block -- counterpart of
``fourierflow.routines.Grid2DMarkovExperiment`` (reference routines/grid_2d_markov.py:23-193, 374-390)
without Lightning / wandb / jax: feature build (positional channels, running normaliser, Gaussian noise),
the operator, inverse-normalise + relative-L2 loss, the manual optimisation step
(routines/base.py:27-52), epoch-0 statistics accumulation, the autoregressive rollout used by predict/infer, and the
trajectory validation / test metrics of ``_valid_step`` / ``compute_losses`` / ``validation_step`` / ``test_step`` (:195-416),
with ``downsample_corr=True`` including the correlation on the reduced grid of ``corr_data`` (:350-370, utils/array.py:18-80),
and with ``pred_path`` the export of the test predictions (:427-476): vorticity, vx, vy on the ``pred_size`` grid and their energy
spectrum, returned by ``test_step`` and written by ``write_predictions``.

Everything on the device is a HIP kernel of libffno_hip.so; torch supplies memory, the stream and the
Gaussian noise samples.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _capi, _lib, diagnostics
from .._lib import ptr as _p
from ..modules.normalizer import Normalizer
from .checkpoint import CheckpointMixin, reject_unsupported_routine_kwargs
from .optimizer import OptimizerMixin


class Grid2DMarkovExperiment(OptimizerMixin, CheckpointMixin, nn.Module):
    def __init__(self, conv: nn.Module, n_steps: Optional[int] = None, low: float = 0, high: float = 1,
                 use_position: bool = True, append_force: bool = False, append_mu: bool = False,
                 max_accumulations: float = 1e6, should_normalize: bool = True, use_fourier_position: bool = False,
                 noise_std: float = 0.0, shuffle_grid: bool = False, use_velocity: bool = False,
                 learn_difference: bool = False, step_size: float = 1.0, optimizer: Optional[dict] = None,
                 scheduler: Optional[dict] = None, domain=((0.0, 2 * math.pi), (0.0, 2 * math.pi)), grid_size=(64,),
                 downsample_corr: bool = False, pred_path: Optional[str] = None, pred_size: int = 64, **unused):
        super().__init__()
        reject_unsupported_routine_kwargs(unused)
        if use_fourier_position:
            raise NotImplementedError("use_fourier_position=True is not built: the reference's own Markov routine cannot run it "
                                      "either (encode_positions reads self.k_max, which its constructor never sets: "
                                      "grid_2d_markov.py:23-45,116)")
        self.conv = conv
        self.shuffle_grid = bool(shuffle_grid)
        if self.shuffle_grid:       # torus_li/ablation/shuffle_xy_grid: fixed random row / column permutations around the model
            assert len(grid_size) == 1, 'shuffle_grid only supports one size'         # grid_2d_markov.py:75-80
            for name, idx in (("x", torch.randperm(grid_size[0])), ("y", torch.randperm(grid_size[0]))):
                self.register_buffer(f"_{name}_idx", idx, persistent=False)            # plain attributes in the reference:
                self.register_buffer(f"_{name}_inv", torch.argsort(idx), persistent=False)   # not part of the state_dict
        self.use_position, self.append_force, self.append_mu = bool(use_position), bool(append_force), bool(append_mu)
        self.n_steps, self.low, self.high = n_steps, low, high
        self.step_size = float(step_size)      # physical time per model step: `time_until` = diverged step * step_size (:348)
        self.should_normalize, self.noise_std, self.learn_difference = should_normalize, noise_std, learn_difference
        self.normalizer = Normalizer([conv.input_dim], max_accumulations)
        self.register_buffer('_float', torch.FloatTensor([0.1]))
        self.use_velocity, self.domain = use_velocity, tuple(tuple(float(v) for v in d) for d in domain)
        if use_velocity:
            # same buffers as the reference (grid_2d_markov.py:82-94) so its checkpoints load strictly; the HIP kernel
            # derives the wavenumbers from the domain lengths itself
            for size in grid_size:
                lx, ly = self.domain[0][1] - self.domain[0][0], self.domain[1][1] - self.domain[1][0]
                kx, ky = np.meshgrid(np.fft.fftfreq(size, d=lx / size), np.fft.rfftfreq(size, d=ly / size), indexing="ij")
                lap = (2 * np.pi * 1j) ** 2 * (np.abs(kx) ** 2 + np.abs(ky) ** 2)
                lap[0, 0] = 1
                self.register_buffer(f'kx_{size}', torch.from_numpy(kx.astype(np.float32)))
                self.register_buffer(f'ky_{size}', torch.from_numpy(ky.astype(np.float32)))
                self.register_buffer(f'lap_{size}', torch.from_numpy(lap.astype(np.complex64)))
        self._vel_ws = None
        # corr_data of another grid size than the model's: reduce every prediction to it on the device (ffno_vorticity_coarsen_step)
        # where the reference calls downsample_vorticity; off, such a batch is refused as before
        self.downsample_corr = bool(downsample_corr)
        # the reference's argument: with it, test_step also exports every prediction on the pred_size x pred_size grid (the
        # reference's hard-coded 64: :433) with its energy spectrum; write_predictions writes them.  validation_step never does.
        self.pred_path = None if pred_path is None else str(pred_path)
        self.pred_size = diagnostics.check_size(pred_size, "pred_size")
        # the F-FNO configs run cosine-with-warm-up per step; the FNOZongyi2DBlock ablations (torus_li/ablation/zongyi_markov*)
        # run StepLR per EPOCH
        self._init_optimizer(optimizer, scheduler, lr=2.5e-3, step_size=100, num_training_steps=100000)
        self._derived = None
        self._partial = None
        self._affine = None

    # ----------------------------------------------------------------------------------------------
    def _build_features(self, batch: Dict[str, torch.Tensor], noise: Optional[torch.Tensor] = None,
                        add_noise: bool = True) -> torch.Tensor:
        """x [B, M, N, Cx] -> normalised features [B, M, N, Cx + 2] (+ noise), accumulating the running
        statistics while training (grid_2d_markov.py:124-170, normalizer.py:45-55)."""
        x = batch['x'].contiguous()
        _lib.require_device_tensor(x, "batch['x']")
        if self.use_velocity:       # [B, M, N, 1] vorticity -> [B, M, N, 3] (vorticity, u, v)  (grid_2d_markov.py:130-144)
            vel = batch.get('velocity')      # the same launch's output for this very x, where the caller holds it already
            x = self._velocity(x) if vel is None else vel
        B, M, N, Cx = x.shape
        extra, keep = None, []
        if not self.use_position or self.append_force or self.append_mu:      # grid_2d_markov.py:146-162
            force = batch['f'].contiguous().float() if self.append_force else None
            mu = batch['mu'].contiguous().float() if self.append_mu else None
            for t, shape in ((force, (B, M, N)), (mu, (B,))):
                if t is not None:
                    _lib.require_device_tensor(t, "batch['f'] / batch['mu']")
                    if tuple(t.shape) != shape:
                        raise ValueError(f"expected a tensor of shape {shape}, got {tuple(t.shape)}")
            keep = [force, mu]
            extra = ctypes.byref(_capi.MarkovExtra(_p(force), _p(mu), int(self.use_position), 0))
        D = Cx + (2 if self.use_position else 0) + int(self.append_force) + int(self.append_mu)
        if D != self.conv.input_dim:
            raise ValueError(f"conv.input_dim={self.conv.input_dim} but the features have {D} channels")
        dev = x.device
        if self._derived is None or self._derived.device != dev:
            self._derived = torch.zeros(2 * D, dtype=torch.float32, device=dev)
            self._partial = torch.empty(256 * 32, dtype=torch.float32, device=dev)
        nz = self.normalizer
        acc = self.should_normalize and nz.should_accumulate()
        state = nz.pack_state()
        if not add_noise:
            noise = None
        elif noise is None and self.noise_std:
            noise = torch.randn(B, M, N, D, device=dev)      # `x += randn * noise_std` (grid_2d_markov.py:168)
        out = torch.empty(B, M, N, D, dtype=torch.float32, device=dev)

        def features(state, accumulate):
            rc = _lib.get_lib().ffno_markov_features(_p(x), _p(state), _p(self._derived), _p(noise), _p(out), _p(self._partial),
                                                     B, M, N, Cx, float(self.low), float(self.high), float(self.noise_std),
                                                     self._eps(), int(accumulate),
                                                     int(self.should_normalize), extra, _lib.current_stream(dev))
            _capi.check(rc, "markov_features")

        features(state, acc)
        if acc:
            nz.unpack_state(state)
            nz._n_acc_host += 1.0
            # data parallel: every rank accumulated its own shard.  Sum the increments over ranks FIRST, then normalise this very
            # batch once more with the statistics of the GLOBAL batch stream (a second pass over 1.5 MB), so that all ranks
            # normalise every step -- this one included -- with identical mean / std, the loss's inverse affine (read from
            # `_derived`) is the global one as well, and any rank's checkpoint holds the full statistics.
            if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                    torch.distributed.get_world_size() > 1:
                nz.sync_across_ranks()
                features(nz.pack_state(), False)
        del keep
        return out

    def _velocity(self, x: torch.Tensor) -> torch.Tensor:
        B, M, N, Cx = x.shape
        if Cx != 1:
            raise ValueError("use_velocity expects the single-channel vorticity field [B, M, N, 1]")
        lib = _lib.get_lib()
        need = int(lib.ffno_velocity_ws_floats(B, M, N))
        if self._vel_ws is None or self._vel_ws.numel() < need or self._vel_ws.device != x.device:
            self._vel_ws = torch.empty(need, dtype=torch.float32, device=x.device)
        out = torch.empty(B, M, N, 3, dtype=torch.float32, device=x.device)
        lx, ly = self.domain[0][1] - self.domain[0][0], self.domain[1][1] - self.domain[1][0]
        _capi.check(lib.ffno_velocity_features(_p(x), _p(out), _p(self._vel_ws), B, M, N, lx, ly,
                                               _lib.current_stream(x.device)), "velocity_features")
        return out

    def _eps(self) -> float:
        if not hasattr(self, "_eps_host"):
            self._eps_host = float(self.normalizer.std_epsilon.flatten()[0].item())   # one sync, at first use
        return self._eps_host

    def _affine_tensor(self):
        """{std[0], mean[0]} for Normalizer.inverse(channel=0) fused into the loss kernel."""
        if not self.should_normalize:
            return None
        D = self.conv.input_dim
        self._affine = torch.stack([self._derived[D], self._derived[0]]).contiguous()
        return self._affine

    def _training_step(self, batch, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """features -> conv -> inverse-normalise -> LpLoss.rel, then the manual optimisation step."""
        tr = self.trainer()
        feats = self._build_features(batch, noise)
        targets = (batch['dy'] if self.learn_difference else batch['y']).contiguous()
        pred = self._unshuffle(tr.engine.forward(self._shuffle(feats), True))
        loss, gy = tr.loss_and_grad(pred, targets, self._affine_tensor())
        tr.apply_gradients(tr.engine.backward(self._shuffle(gy)))      # adjoint of the inverse gather = the forward gather
        return loss

    @torch.no_grad()
    def pair_loss(self, batch) -> torch.Tensor:
        """The loss of one x / y pair batch without an optimisation step: features (no noise) -> conv on the inference engine ->
        inverse-normalise -> LpLoss.rel.  Under eval() the normaliser statistics stand still."""
        tr = self.trainer()
        pred = self._unshuffle(tr.engine.forward(self._shuffle(self._build_features(batch, add_noise=False)), False))
        target = (batch['dy'] if self.learn_difference else batch['y']).contiguous()
        return tr.loss_and_grad(pred, target, self._affine_tensor())[0]

    def _shuffle(self, t: torch.Tensor) -> torch.Tensor:
        """x[:, x_idx][:, :, y_idx] (grid_2d_markov.py:177-178)."""
        if not self.shuffle_grid:
            return t
        return t.index_select(1, self._x_idx).index_select(2, self._y_idx).contiguous()

    def _unshuffle(self, t: torch.Tensor) -> torch.Tensor:
        """im[:, :, y_inv][:, x_inv] (grid_2d_markov.py:182-183)."""
        if not self.shuffle_grid:
            return t
        return t.index_select(2, self._y_inv).index_select(1, self._x_inv).contiguous()

    def training_step(self, batch, epoch: int, noise: Optional[torch.Tensor] = None):
        """Epoch 0 only accumulates the normaliser statistics (grid_2d_markov.py:376-378); later epochs train."""
        self.current_epoch = int(epoch)
        if self.should_normalize and epoch < 1:
            with torch.no_grad():
                self._build_features(batch, noise)
            return None
        return self._training_step(batch, noise)

    @torch.no_grad()
    def rollout(self, x0: torch.Tensor, n_steps: Optional[int] = None, f: Optional[torch.Tensor] = None,
                mu: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Autoregressive inference (grid_2d_markov.py:263-321): feed each de-normalised prediction back as the
        next input (the force map ``f`` [B, M, N] and viscosity ``mu`` [B] stay fixed).  x0 [B, M, N, 1] -> [B, M, N, n_steps]."""
        was_training = self.normalizer.training
        self.normalizer.eval()
        tr = self.trainer()
        preds, x, prev = [], x0, x0
        for _ in range(n_steps or self.n_steps or 1):
            feats = self._build_features({'x': x, 'f': f, 'mu': mu}, add_noise=False)   # no noise at validation (:292-293)
            im = self._unshuffle(tr.engine.forward(self._shuffle(feats), False))      # :297-304
            if self.should_normalize:
                D = self.conv.input_dim
                im = im * self._derived[D] + self._derived[0]
            if self.learn_difference:
                im = prev + im
                prev = im
            preds.append(im)
            x = im
        self.normalizer.train(was_training)
        return torch.cat(preds, dim=-1)

    @torch.no_grad()
    def simulate(self, x0: torch.Tensor, n_steps: int, f: Optional[torch.Tensor] = None, mu: Optional[torch.Tensor] = None,
                 every: int = 1) -> torch.Tensor:
        """The trained model as a simulator: n_steps autoregressive steps from x0 [B, M, N] (or [B, M, N, 1]), every `every`-th
        state kept -> [B, M, N, n_steps / every] (column j is the state after (j + 1) * every steps; n_steps is a multiple of
        `every`, so that the columns are evenly spaced in time).  ``f`` is one force map [B, M, N] or a stack [B, M, N, T' >=
        n_steps] whose column t drives step t (read in place, strided); ``mu`` is [B].

        The feature kernel runs once, on x0, in eval mode: the statistics stand still.  Every step is then the inference engine
        and ONE ffno_markov_advance launch (inverse normalisation, difference update, the running field in place, the trajectory
        column, the next step's features written straight into the engine's input buffer).  The trajectory is allocated once.
        With `use_velocity` or `shuffle_grid` the launch only updates the field and the trajectory, and the velocity / feature
        / gather launches of `_valid_step` build the next input from the field.  The numbers are those of `_valid_step`, bit
        for bit: the same engine on the same inputs, the same fused order of the inverse affine."""
        n_steps, every = int(n_steps), int(every)
        if n_steps < 1 or every < 1 or n_steps % every:
            raise ValueError(f"simulate needs n_steps >= 1 and every >= 1 dividing n_steps, got n_steps={n_steps}, every={every}")
        _lib.require_device_tensor(x0, "x0")
        if x0.dim() == 4 and x0.shape[-1] == 1:
            x0 = x0[..., 0]
        if x0.dim() != 3:
            raise ValueError(f"x0 must be [B, M, N] or [B, M, N, 1], got {tuple(x0.shape)}")
        B, M, N = x0.shape
        dev, lib, stream = x0.device, _lib.get_lib(), _lib.current_stream(x0.device)
        force = mu_t = None
        if self.append_force:
            if f is None or f.dim() not in (3, 4) or tuple(f.shape[:3]) != (B, M, N) or (f.dim() == 4 and f.shape[-1] < n_steps):
                raise ValueError(f"f must be [{B}, {M}, {N}] or [{B}, {M}, {N}, >= {n_steps}], got "
                                 f"{None if f is None else tuple(f.shape)}")
            _lib.require_device_tensor(f, "f")
            force = f.float()
            # a pixel-uniform stride is all the kernel needs: a slice of a contiguous stack along time is read where it lies
            s = force.stride(2) if force.dim() == 4 else 1
            if force.dim() == 3 or s < 1 or tuple(force.stride()[:3]) != (M * N * s, N * s, s):
                force = force.contiguous()
        if self.append_mu:
            if mu is None or tuple(mu.shape) != (B,):
                raise ValueError(f"mu must be [{B}], got {None if mu is None else tuple(mu.shape)}")
            _lib.require_device_tensor(mu, "mu")
            mu_t = mu.contiguous().float()
        stack = force is not None and force.dim() == 4
        f_stride = force.stride(2) if stack else 1

        def f_at(t):      # the map of step t as `_build_features` takes it
            return force[..., t].contiguous() if stack else force

        def f_ptr(t):
            if force is None:
                return None
            return force.data_ptr() + 4 * t * force.stride(3) if stack else force.data_ptr()

        field = torch.empty(B, M, N, 1, dtype=torch.float32, device=dev)      # the running field, updated in place
        field.copy_(x0.unsqueeze(-1))
        traj = torch.empty(B, M, N, n_steps // every, dtype=torch.float32, device=dev)
        fused = not (self.use_velocity or self.shuffle_grid)
        tr = self.trainer()
        view = {"own_output": False} if tr.engine.can_return_view else {}
        D = self.conv.input_dim
        was_training = self.normalizer.training
        self.normalizer.eval()
        try:
            feats = self._build_features({'x': field, 'f': f_at(0) if force is not None else None, 'mu': mu_t}, add_noise=False)
            affine = self._affine_tensor()
            desc = _capi.MarkovAdvanceDesc(affine=_p(affine), prev=_p(field) if self.learn_difference else None,
                                           derived=_p(self._derived), mu=_p(mu_t), force_stride=f_stride,
                                           L=traj.shape[-1], D=D, use_position=int(self.use_position),
                                           normalize=int(self.should_normalize), low=float(self.low), high=float(self.high))
            for t in range(n_steps):
                if not fused and t > 0:
                    feats = self._build_features({'x': field, 'f': f_at(t) if force is not None else None, 'mu': mu_t},
                                                 add_noise=False)
                if fused:      # (the engine's own output buffer: the launch below consumes it before the next pass)
                    out = tr.engine.forward(feats, False, **view)
                else:
                    out = self._unshuffle(tr.engine.forward(self._shuffle(feats), False))
                if tuple(out.shape) != (B, M, N, 1):
                    raise ValueError(f"the rollout feeds one predicted channel back, conv returned {tuple(out.shape)}")
                keep = (t + 1) % every == 0
                desc.traj, desc.col = (_p(traj) if keep else None), ((t + 1) // every - 1 if keep else 0)
                build = fused and t + 1 < n_steps
                desc.feats, desc.force = (_p(feats) if build else None), (f_ptr(t + 1) if build else None)
                _capi.check(lib.ffno_markov_advance(_p(out), _p(field), ctypes.byref(desc), B, M, N, stream), "markov_advance")
        finally:
            self.normalizer.train(was_training)
        return traj

    # -- trajectory validation (grid_2d_markov.py:195-416) ---------------------------------------------------------------------
    def _traj_geometry(self, data: torch.Tensor):
        B, M, N, T = data.shape
        n_steps = self.n_steps or T - 1
        if not 0 < n_steps < T:
            raise ValueError(f"n_steps={n_steps} needs a trajectory of at least {n_steps + 1} steps, batch['data'] has {T}")
        return B, M, N, T, n_steps

    @torch.no_grad()
    def _valid_step(self, batch: Dict[str, torch.Tensor], export: bool = False):
        """Autoregressive rollout over batch['data'] [B, M, N, T] from data[..., T - n_steps - 1] (:195-326) ->
        (summed step loss, step_losses [n_steps], preds [B, M, N, n_steps], []).  No noise, no statistics accumulation.  Per step:
        the feature kernel, the inference engine, one ffno_markov_traj_step launch (inverse normalisation, difference
        update, next input, preds column and the sums of every metric); ffno_markov_traj_metrics after the loop.  The last
        entry is the reference's `forecast_list` per step, which the inference engine does not produce.  With `export` (test_step of a
        routine with a pred_path) every step also makes one ffno_prediction_export_step launch on the velocity image of its
        prediction, and one batched rfft2 with one ffno_energy_spectrum launch follows the loop: `self._pred`."""
        data = batch['data'].contiguous().float()
        _lib.require_device_tensor(data, "batch['data']")
        B, M, N, T, n_steps = self._traj_geometry(data)
        dev, lib, stream = data.device, _lib.get_lib(), _lib.current_stream(data.device)
        force = batch['f'].float() if self.append_force else None
        if force is not None and force.dim() == 4:      # [B, M, N, T']: the last n_steps maps, one per step (:245-247)
            force = force[..., -n_steps:]
            if force.shape[-1] != n_steps:
                raise ValueError(f"batch['f'] holds {force.shape[-1]} force maps, the rollout needs {n_steps}")
        mu = batch['mu'] if self.append_mu else None
        sums = torch.empty(int(lib.ffno_markov_traj_ws_floats(B, M, N, n_steps)), dtype=torch.float32, device=dev)
        corr = self._reduced_corr(batch, B, M, N, n_steps)      # None: corr_data absent, of the grid's own size, or the switch off
        metrics = torch.empty(4 + 2 * n_steps + (2 + n_steps if corr is not None else 0), dtype=torch.float32, device=dev)
        sums2 = self._coarsen_sums(corr, B, n_steps)
        preds = torch.empty(B, M, N, n_steps, dtype=torch.float32, device=dev)
        slabs = self._export_slabs(B, M, N, n_steps, dev) if export else None
        im = data[..., T - n_steps - 1].unsqueeze(-1).contiguous()      # the first input; then every prediction, in place
        prev = _p(im) if self.learn_difference else None                 # prev_im is the running field itself (:316-318)
        tr = self.trainer()
        was_training = self.normalizer.training
        self.normalizer.eval()
        try:
            affine = vel = None
            for t in range(n_steps):
                f_t = force if force is None or force.dim() == 3 else force[..., t].contiguous()
                feats = self._build_features({'x': im, 'f': f_t, 'mu': mu, 'velocity': vel}, add_noise=False)
                if t == 0:      # the statistics stand still during validation: one inverse affine for the whole rollout
                    affine = self._affine_tensor()
                out = self._unshuffle(tr.engine.forward(self._shuffle(feats), False))
                if tuple(out.shape) != (B, M, N, 1):
                    raise ValueError(f"the rollout feeds one predicted channel back, conv returned {tuple(out.shape)}")
                _capi.check(lib.ffno_markov_traj_step(_p(out), _p(affine), prev, _p(data), _p(im), _p(preds), _p(sums),
                                                      B, M, N, T, n_steps, t, stream), "markov_traj_step")
                if corr is not None or slabs is not None:      # the velocity image of this prediction, computed once: reduced
                    vel = self._velocity(im)                   # and exported here, and the next step's features
                    if corr is not None:
                        self._coarsen_step(vel, corr, sums2, n_steps, t)
                    if slabs is not None:
                        self._export_step(vel, slabs, n_steps, t)
                    if not self.use_velocity:
                        vel = None
        finally:
            self.normalizer.train(was_training)
        _capi.check(lib.ffno_markov_traj_metrics(_p(sums), _p(metrics), B, M, N, n_steps, 0.95, stream), "markov_traj_metrics")
        if corr is not None:
            self._corr_metrics(sums2, metrics, corr, B, n_steps)
        self._traj = (preds, metrics, corr is not None)
        self._pred = None
        if slabs is not None:      # [3][n_steps][B][m][m]: vorticity, vx, vy
            self._pred = dict(zip(diagnostics.PRED_KEYS, (*slabs.unbind(0), diagnostics._spectrum_of_pair(slabs[1:]))))
        step_losses = metrics[4:4 + n_steps]
        return step_losses.sum(), step_losses, preds, []

    @torch.no_grad()
    def compute_losses(self, batch: Dict[str, torch.Tensor], loss, preds: torch.Tensor):
        """(loss / n_steps, loss_full, time_until, reduced_time_until, p, times) of :328-372.  For the `preds` of the last
        `_valid_step` everything was reduced on the device already; any other `preds` goes through the same two kernels
        (their sums 2..5 depend on the predictions alone).  One host read: `self.last_metrics`."""
        data = batch['data'].contiguous().float()
        B, M, N, T, n_steps = self._traj_geometry(data)
        if 'corr_data' in batch and batch['corr_data'].shape[1] != M and not self.downsample_corr:
            raise NotImplementedError("corr_data of another grid size needs downsample_vorticity (jax-cfd), which is not built: "
                                      "pass corr_data at the model's own resolution, or build the routine with downsample_corr=True "
                                      "to reduce the predictions on the device (ffno_vorticity_coarsen_step)")
        corr = self._reduced_corr(batch, B, M, N, n_steps)
        base = 4 + 2 * n_steps      # where the reduced numbers { diverged_t, mean_t p_2, p_2[n_steps] } follow the full ones
        cached = getattr(self, "_traj", None)
        if cached is not None and cached[0] is preds and cached[2] == (corr is not None):
            metrics = cached[1]
            loss = metrics[0]
        else:
            if tuple(preds.shape) != (B, M, N, n_steps):
                raise ValueError(f"preds must be {(B, M, N, n_steps)}, got {tuple(preds.shape)}")
            _lib.require_device_tensor(preds, "preds")
            lib, stream = _lib.get_lib(), _lib.current_stream(data.device)
            sums = torch.empty(int(lib.ffno_markov_traj_ws_floats(B, M, N, n_steps)), dtype=torch.float32, device=data.device)
            metrics = torch.empty(base + (2 + n_steps if corr is not None else 0), dtype=torch.float32, device=data.device)
            sums2 = self._coarsen_sums(corr, B, n_steps)
            im, again = torch.empty(B, M, N, dtype=torch.float32, device=data.device), torch.empty_like(preds)
            for t in range(n_steps):
                col = preds[..., t].contiguous().float()
                _capi.check(lib.ffno_markov_traj_step(_p(col), None, None, _p(data), _p(im), _p(again), _p(sums),
                                                      B, M, N, T, n_steps, t, stream), "markov_traj_step")
                if corr is not None:
                    self._coarsen_step(self._velocity(col.unsqueeze(-1)), corr, sums2, n_steps, t)
            _capi.check(lib.ffno_markov_traj_metrics(_p(sums), _p(metrics), B, M, N, n_steps, 0.95, stream), "markov_traj_metrics")
            if corr is not None:
                self._corr_metrics(sums2, metrics, corr, B, n_steps)
            loss = loss / n_steps
        host = metrics.cpu()
        self.last_metrics = host
        time_until = float(host[2]) * self.step_size
        times = batch['times'][0, -n_steps:] if 'times' in batch else None
        if corr is not None:      # p is p_2, and the logged mean correlation with it; time_until stays the full one (:358-372)
            self.last_corr = float(host[base + 1])
            return loss, metrics[1], time_until, float(host[base]) * self.step_size, metrics[base + 2:], times
        # corr_data at the grid's own size: the reduced metrics ARE the full ones (:351-357)
        self.last_corr = float(host[3])
        return loss, metrics[1], time_until, time_until, metrics[4 + n_steps:base], times

    # -- the correlation on the grid of corr_data (:350-370) -------------------------------------------------------------------
    def _reduced_corr(self, batch, B: int, M: int, N: int, n_steps: int) -> Optional[torch.Tensor]:
        """batch['corr_data'] [B, m, m, Tc] where the predictions have to be reduced to its grid, else None."""
        if not self.downsample_corr or 'corr_data' not in batch or batch['corr_data'].shape[1] == M:
            return None
        corr = batch['corr_data']
        _lib.require_device_tensor(corr, "batch['corr_data']")
        shape = tuple(corr.shape)
        if corr.dim() != 4 or shape[0] != B:
            raise ValueError(f"batch['corr_data'] must be [{B}, m, m, Tc], got {shape}")
        if shape[1] != shape[2]:
            raise ValueError(f"batch['corr_data'] {shape} is not square: the reduction of a {M} x {N} prediction takes one factor "
                             f"for both directions")
        m = shape[1]
        if M % m or N % m or M // m != N // m:
            raise ValueError(f"batch['corr_data'] {shape}: a {M} x {N} prediction is reduced by an integer factor, the same in both "
                             f"directions, and {M} / {m}, {N} / {m} is none")
        if shape[3] < n_steps:
            raise ValueError(f"batch['corr_data'] {shape} holds {shape[3]} steps, the rollout of batch['data'] "
                             f"{tuple(batch['data'].shape)} compares {n_steps}")
        return corr.contiguous().float()

    def _coarsen_sums(self, corr, B: int, n_steps: int) -> Optional[torch.Tensor]:
        if corr is None:
            return None
        n = int(_lib.get_lib().ffno_vorticity_coarsen_ws_floats(B, corr.shape[1], n_steps))
        if n == 0:
            raise ValueError(f"batch['corr_data'] {tuple(corr.shape)}: grid size outside ffno_vorticity_coarsen_step's range")
        return torch.empty(n, dtype=torch.float32, device=corr.device)

    def _coarsen_step(self, vel: torch.Tensor, corr: torch.Tensor, sums2: torch.Tensor, n_steps: int, t: int):
        B, M, N, _ = vel.shape
        lx, ly = self.domain[0][1] - self.domain[0][0], self.domain[1][1] - self.domain[1][0]
        _capi.check(_lib.get_lib().ffno_vorticity_coarsen_step(_p(vel), _p(corr), None, _p(sums2), B, M, N, corr.shape[1],
                                                               corr.shape[3], n_steps, t, lx, ly,
                                                               _lib.current_stream(vel.device)), "vorticity_coarsen_step")

    def _corr_metrics(self, sums2: torch.Tensor, metrics: torch.Tensor, corr: torch.Tensor, B: int, n_steps: int):
        tail = ctypes.c_void_p(metrics.data_ptr() + 4 * (4 + 2 * n_steps))
        _capi.check(_lib.get_lib().ffno_markov_corr_metrics(_p(sums2), tail, B, corr.shape[1], n_steps, 0.95,
                                                            _lib.current_stream(metrics.device)), "markov_corr_metrics")

    # -- the export behind pred_path (:427-476) ----------------------------------------------------------------------------------
    def _export_slabs(self, B: int, M: int, N: int, n_steps: int, dev) -> torch.Tensor:
        m = self.pred_size
        if M % m or N % m or M // m != N // m:
            raise ValueError(f"pred_path: a {M} x {N} prediction is exported on the {m} x {m} grid of pred_size={m} by an integer "
                             f"factor, the same in both directions, and {M} / {m}, {N} / {m} is none (the reference writes a file "
                             f"with the axes of a 64 x 64 grid whatever the model's)")
        return torch.empty(3, n_steps, B, m, m, dtype=torch.float32, device=dev)

    def _export_step(self, vel: torch.Tensor, slabs: torch.Tensor, n_steps: int, t: int):
        B, M, N, _ = vel.shape
        lx, ly = self.domain[0][1] - self.domain[0][0], self.domain[1][1] - self.domain[1][0]
        _capi.check(_lib.get_lib().ffno_prediction_export_step(_p(vel), _p(slabs[0]), _p(slabs[1]), _p(slabs[2]), B, M, N,
                                                               self.pred_size, n_steps, t, lx, ly,
                                                               _lib.current_stream(vel.device)), "prediction_export_step")

    def write_predictions(self, path: Optional[str], parts, times=None) -> str:
        """The `pred_*` arrays of the test batches `parts` as one file, the .npz sibling of `path` (default: this routine's
        pred_path): diagnostics.write_predictions with this routine's domain and step size.  The reference's test_step overwrites
        its file with every batch, so that only the last batch survives; here writing is a step of its own, once per split."""
        path = self.pred_path if path is None else path
        if path is None:
            raise ValueError("write_predictions needs a path: the routine was built without pred_path")
        return diagnostics.write_predictions(path, parts, times, domain=self.domain, step_size=self.step_size)

    def _trajectory_metrics(self, batch, export: bool = False):
        loss, step_losses, preds, _ = self._valid_step(batch, export)
        loss, loss_full, time_until, reduced, p, times = self.compute_losses(batch, loss, preds)
        return loss, loss_full, time_until, reduced, p, times, step_losses

    def validation_step(self, batch, batch_idx: int = 0):
        """The reference's logged validation keys (:392-406); a NaN loss becomes 9999.9 so that checkpoint selection by
        `valid_loss` never prefers a diverged model."""
        loss, loss_full, time_until, reduced, p, _, _ = self._trajectory_metrics(batch)
        host = self.last_metrics
        if math.isnan(float(host[0])):
            loss = 9999.9
        if math.isnan(float(host[1])):
            loss_full = 9999.9
        return {'valid_loss_avg': loss, 'valid_loss': loss_full, 'valid_time_until': time_until,
                'valid_reduced_time_until': reduced, 'valid_corr': self.last_corr}

    def test_step(self, batch, batch_idx: int = 0):
        """The reference's logged test keys (:408-425); its two wandb tables are returned as `test_correlations` (p per step)
        and `test_losses` (relative-L2 per step), with `test_times` when the batch carries `times`.  A routine with a pred_path
        adds pred_vorticity, pred_vx, pred_vy [n_steps, B, pred_size, pred_size] and pred_energy_spectrum
        [n_steps, B, pred_size / 2 + 1], device tensors (:427-476); it writes nothing -- see write_predictions."""
        loss, loss_full, time_until, reduced, p, times, step_losses = self._trajectory_metrics(batch, self.pred_path is not None)
        out = {'test_loss_avg': loss, 'test_loss': loss_full, 'test_time_until': time_until,
               'test_reduced_time_until': reduced, 'test_corr': self.last_corr,
               'test_correlations': p, 'test_losses': step_losses}
        if times is not None:
            out['test_times'] = times
        if self._pred is not None:
            out.update(self._pred)
        return out
