"""Host driver of the FNOZongyi2DBlock baseline (BASELINE config 0).

Reference: fourierflow/modules/zongyi_fno/grid_2d.py:16-78 (SpectralConv2d: rfft2 -> two K x K corner blocks ->
irfft2, plus a pointwise linear, ReLU) and :81-129 (FNOZongyi2DBlock: in_proj, n_layers of those, a
Linear-ReLU-Linear head).  The spectral convolution is the same operator as FNOPlus2DBlock's, so it runs on the same
kernels, the corner chain of _corner_chain.py; everything
pointwise runs on csrc/plin.hip.  The baseline is 20 channels wide: activations and weights live in buffers padded
to the 32- (or 64-) channel tiles of the spectral kernels with exact zeros in the pad, one ffno_pad_copy launch
moves all parameters into their padded twins before a pass and all gradients back after it.

Unlike the F-FNO engine this one returns the INPUT gradient as well and keeps several forward passes alive at once
(``slot``): Grid2DRolloutExperiment back-propagates through a 10-step autoregressive rollout
(routines/grid_2d_rollout.py:104-134).
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _capi, _lib
from ._corner_chain import CornerChain
from ._engine_core import EngineCore

_p = _lib.ptr
HEAD_DIM = 128


class ZongyiEngine(EngineCore):
    def __init__(self, *, modes: int, width: int, input_dim: int, n_layers: int, residual: bool = False,
                 conv_residual: bool = True):
        if width > 32:
            raise NotImplementedError("FNOZongyi2DBlock: width > 32 is outside the compiled tile set of the baseline path")
        self.K, self.W, self.Cin, self.L = modes, width, input_dim, n_layers
        # residual: x = layer(x) + x (grid_2d.py:126);  conv_residual: act(spectral(x) + linear(x)), else
        # act(linear(spectral(x))) (grid_2d.py:74-77) -- torus_li/ablation/zongyi_markov_residual uses (True, False)
        self.residual, self.conv_residual = bool(residual), bool(conv_residual)
        self.C = 32            # channel tile of the spectral kernels; channels width..31 are exact zeros
        self.O = 1
        self.Ktot = 2 * modes * modes      # retained (ky, kx') modes: one [2][C][C] block of the planes each
        W, K, C = width, modes, self.C
        params = [("in_proj.weight", (W, input_dim), (W, input_dim, 1, C, input_dim)),
                  ("in_proj.bias", (W,), (1, W, 1, 1, C))]
        for l in range(n_layers):
            pre = f"spectral_layers.{l}."
            params += [(pre + "linear.weight", (W, W), (W, W, 1, C, C)),
                       (pre + "linear.bias", (W,), (1, W, 1, 1, C))]
            params += [(pre + f"fourier_weight.{j}", (W, W, K, K, 2), (W, W, K * K * 2, C, C)) for j in range(2)]
        params += [("feedforward.0.weight", (HEAD_DIM, W), (HEAD_DIM, W, 1, HEAD_DIM, C)),
                   ("feedforward.0.bias", (HEAD_DIM,), (1, HEAD_DIM, 1, 1, HEAD_DIM)),
                   ("feedforward.2.weight", (1, HEAD_DIM), (1, HEAD_DIM, 1, 1, HEAD_DIM)),
                   ("feedforward.2.bias", (1,), (1, 1, 1, 1, 1))]
        self._register(params)
        self._reset_state()

    def _register(self, params):
        """``params``: (name, shape, pad geometry) in registration order; the pad geometry is (R, Cc, inner) of the plain tensor
        and (Rp, Cp) of its padded twin.  Lays out the flat gradient buffer and the padded twins."""
        self._lay_out({n: shape for n, shape, _ in params})
        self._pad_geom = {n: geom for n, _, geom in params}
        self._poffsets, poff = {}, 0
        for n in self.param_names:
            R, Cc, inner, Rp, Cp = self._pad_geom[n]
            self._poffsets[n] = poff
            poff += Rp * Cp * inner
        self.n_padded = poff

    def _reset_state(self):
        """The state of an engine nothing is bound to yet."""
        self.params: Dict[str, torch.Tensor] = {}
        self.device = None
        self.timer = None
        self._issue_stream = 0
        self.paired_last = False
        self._ws = {}
        self._ptr_sig = None
        self._bound_sig = None      # data pointers of the tensors bound last
        self._packed = False

    # ------------------------------------------------------------------------------------------------
    def bind(self, params: Dict[str, torch.Tensor]):
        dev = self._validate(params)
        sig = tuple(params[n].data_ptr() for n in self.param_names)
        if sig != self._bound_sig:
            self._packed = False          # other tensors: the padded twins are stale whatever the caller says
        self._bound_sig = sig
        self.params = {n: params[n] for n in self.param_names}
        if dev != self.device:
            self.device = dev
            f32 = dict(dtype=torch.float32, device=dev)
            self.gflat = torch.zeros(self.n_params, **f32)
            self.ppad = torch.zeros(self.n_padded, **f32)      # padded parameters (pad entries stay 0 forever)
            self.gpad = torch.zeros(self.n_padded, **f32)      # padded gradients
            n = 2 * self.Ktot * self.C * self.C
            self.planes = [(torch.empty(n, **f32), torch.empty(n, **f32)) for _ in range(self.L)]
            self._ws = {}
        self._ptr_sig = None

    def zero_grad(self):
        """Start a fresh accumulation for backward(..., accumulate=True)."""
        self.gpad.zero_()
        self.gflat.zero_()

    def _aliased(self, name) -> bool:
        """The padded twin has the parameter's own shape (width == channel tile): use the tensor itself, no copy."""
        R, Cc, inner, Rp, Cp = self._pad_geom[name]
        return R == Rp and Cc == Cp

    def _pp(self, name, buf=None) -> torch.Tensor:
        R, Cc, inner, Rp, Cp = self._pad_geom[name]
        if self._aliased(name):
            return (self.params[name] if buf is None else self.grad_view(name)).reshape(-1)
        o = self._poffsets[name]
        return (self.ppad if buf is None else buf)[o:o + Rp * Cp * inner]

    def _refresh_pointers(self):
        sig = tuple(self.params[n].data_ptr() for n in self.param_names)
        if sig == self._ptr_sig:
            return
        self._ptr_sig = sig

        def table(plain_of, padded_buf):
            descs = []
            for n in self.param_names:
                if self._aliased(n):
                    continue
                R, Cc, inner, Rp, Cp = self._pad_geom[n]
                descs.append(_capi.PadDesc(plain_of(n).data_ptr(), self._pp(n, padded_buf).data_ptr(), R, Cc, inner, Cp))
            self._n_pad = len(descs)
            return _lib.device_table(_capi.PadDesc, descs, self.device) if descs else None

        self._ptab = table(lambda n: self.params[n], self.ppad)
        self._gtab = table(self.grad_view, self.gpad)

    # ------------------------------------------------------------------------------------------------
    def _workspace(self, B, M, N, n_slots):
        key = (B, M, N)
        ws = self._ws.get(key)
        if ws is not None and len(ws.slots) >= n_slots:
            return ws
        lib = _lib.get_lib()
        C, L = self.C, self.L
        f32 = dict(dtype=torch.float32, device=self.device)
        if ws is None:
            if M != N:
                raise ValueError(f"FNOZongyi2DBlock needs a square grid, got {M} x {N}: the reference's "
                                 "irfft2(s=(N, M)) (grid_2d.py:68) fails on anything else")
            if 2 * self.K > M or self.K > N // 2 + 1:
                raise ValueError(f"modes={self.K} does not fit a {M} x {N} grid (the reference fails in its einsum here)")
            ws = type("WS", (), {})()
            P = B * M * N
            ws.P = P
            ws.chain = ch = CornerChain(B, (M, N), (self.K, self.K), C, lambda *a: self._k(*a), self.device)
            ws.scr = ch.scratch(lambda n: torch.empty(n, **f32))
            ws.SY = torch.empty(ch.spec, **f32)             # mixed spectrum
            ws.SX0 = torch.empty(ch.spec, **f32)            # forward spectrum when nothing is saved
            ws.SD = torch.empty(ch.spec, **f32)             # adjoint spectrum dY of the current layer
            ws.S = torch.empty(P, C, **f32)                 # spectral branch output of the current layer
            ws.Xa = [torch.empty(P, C, **f32) for _ in range(2)]     # inference ping-pong
            ws.A0 = torch.empty(P, C, **f32) if self.residual else None   # layer output before the block-level residual
            ws.H0 = torch.empty(P, HEAD_DIM, **f32)
            ws.G = [torch.empty(P, C, **f32) for _ in range(2)]
            ws.DP = torch.empty(P, C, **f32)
            ws.DH = torch.empty(P, HEAD_DIM, **f32)
            ws.fwpart = torch.empty(ch.planes_floats, **f32)
            ws.part = torch.empty(int(lib.ffno_plin_wgrad_partial_floats(P, C, HEAD_DIM)), **f32)
            ws.slots = []
            self._ws[key] = ws
            while len(self._ws) > 3:
                self._ws.pop(next(iter(self._ws)))
        while len(ws.slots) < n_slots:
            s = type("Slot", (), {})()
            s.x = torch.empty(ws.P, self.Cin, **f32)
            s.X = torch.empty(L + 1, ws.P, C, **f32)        # X[0] = in_proj(x), X[l+1] = output of layer l
            s.SX = torch.empty(L, ws.chain.spec, **f32)      # forward 2-D spectra (inputs of the weight gradient)
            s.H = torch.empty(ws.P, HEAD_DIM, **f32)
            s.A = torch.empty(L, ws.P, C, **f32) if self.residual else None          # relu outputs (ReLU masks)
            s.S = torch.empty(L, ws.P, C, **f32) if not self.conv_residual else None # spectral outputs (inputs of `linear`)
            s.live = False
            ws.slots.append(s)
        return ws

    def _prepare_weights(self, st):
        lib = _lib.get_lib()
        self._refresh_pointers()
        self._packed = True
        if self._n_pad:
            self._k("pad_copy", lib.ffno_pad_copy, _p(self._ptab), self._n_pad, 1, st)
        self._pack_planes(lib, st)

    def _pack_planes(self, lib, st):
        for l in range(self.L):
            pre = f"spectral_layers.{l}."
            self._k("fw2d_pack", lib.ffno_fw2d_pack, _p(self._pp(pre + "fourier_weight.0")),
                    _p(self._pp(pre + "fourier_weight.1")), _p(self.planes[l][0]), _p(self.planes[l][1]), self.C, self.K, st)

    # ------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, save_for_backward: bool, slot: int = 0, n_slots: int = 1,
                weights_ready: bool = False) -> torch.Tensor:
        """x [B, M, N, input_dim] -> forecast [B, M, N, 1].  With ``save_for_backward`` the activations are kept in
        ``slot`` until its backward() ran."""
        _lib.require_device_tensor(x, "x")
        if x.dim() != 4 or x.shape[-1] != self.Cin:
            raise ValueError(f"expected x of shape [B, M, N, {self.Cin}], got {tuple(x.shape)}")
        if not self.params:
            raise RuntimeError("bind() the parameters first")
        lib = _lib.get_lib()
        B, M, N, _ = x.shape
        ws = self._workspace(B, M, N, max(n_slots, slot + 1))
        st = _lib.current_stream(self.device)
        self._issue_stream = st
        C, L, P, Cin = self.C, self.L, ws.P, self.Cin
        if not (weights_ready and self._packed):      # weights_ready: the caller vouches the parameters did not change
            self._prepare_weights(st)
        pp = self._pp
        if save_for_backward:
            sl = ws.slots[slot]
            sl.x.copy_(x.reshape(P, Cin))
            xin, X, H = sl.x, sl.X, sl.H
            sl.live = True
        else:
            xin, X, H = x.contiguous().view(P, Cin), None, ws.H0
        cur = X[0] if X is not None else ws.Xa[0]
        self._k("in_proj", lib.ffno_plin_fwd, _p(xin), Cin, _p(pp("in_proj.weight")), _p(pp("in_proj.bias")), None, _p(cur), C,
                None, None, None, P, Cin, C, 0, st)
        for l in range(L):
            pre = f"spectral_layers.{l}."
            nxt = X[l + 1] if X is not None else ws.Xa[(l + 1) & 1]
            S = sl.S[l] if (save_for_backward and not self.conv_residual) else ws.S
            # S = irfft2(corner-mix(rfft2(cur)))   (grid_2d.py:48-71)
            ws.chain.conv(cur, S, sl.SX[l] if save_for_backward else ws.SX0, ws.SY, self.planes[l][0], ws.scr, True, st)
            # conv_residual: act(spectral(x) + linear(x)), else act(linear(spectral(x)))   (grid_2d.py:74-77);
            # block-level residual: x = layer(x) + x as a second output, the ReLU output itself is kept for the mask (:126)
            A = nxt if not self.residual else (sl.A[l] if save_for_backward else ws.A0)
            src, add = (cur, S) if self.conv_residual else (S, None)
            self._k("layer_linear", lib.ffno_plin_fwd, _p(src), C, _p(pp(pre + "linear.weight")), _p(pp(pre + "linear.bias")),
                    _p(add), _p(A), C, _p(cur) if self.residual else None, _p(nxt) if self.residual else None, None, P, C, C, 1, st)
            cur = nxt
        self._k("head_fc1", lib.ffno_plin_fwd, _p(cur), C, _p(pp("feedforward.0.weight")), _p(pp("feedforward.0.bias")), None,
                _p(H), HEAD_DIM, None, None, None, P, C, HEAD_DIM, 1, st)
        y = torch.empty(P, 1, dtype=torch.float32, device=self.device)
        self._k("head_fc2", lib.ffno_plin_fwd, _p(H), HEAD_DIM, _p(pp("feedforward.2.weight")), _p(pp("feedforward.2.bias")),
                None, _p(y), 1, None, None, None, P, HEAD_DIM, 1, 0, st)
        return y.view(B, M, N, 1)

    # ------------------------------------------------------------------------------------------------
    def backward(self, gy: torch.Tensor, slot: int = 0, need_dx: bool = False, accumulate: bool = False):
        """gy = dL/dforecast [B, M, N, 1] for the pass saved in ``slot``.  Fills (or, with ``accumulate``, adds to) the
        flat gradient buffer and returns ``gflat`` -- or ``(gflat, dx)`` with ``need_dx``."""
        _lib.require_device_tensor(gy, "gy")
        lib = _lib.get_lib()
        B, M, N, _ = gy.shape
        ws = self._ws.get((B, M, N))
        if ws is None or slot >= len(ws.slots) or not ws.slots[slot].live:
            raise RuntimeError("backward() needs a preceding forward(save_for_backward=True) in the same slot")
        sl = ws.slots[slot]
        sl.live = False
        gy = gy.contiguous().view(ws.P, 1)
        st = _lib.current_stream(self.device)
        self._issue_stream = st
        C, L, P, Cin = self.C, self.L, ws.P, self.Cin
        pp = self._pp
        gp = lambda n: self._pp(n, self.gpad)       # noqa: E731
        acc = int(bool(accumulate))
        XL = sl.X[L]
        # head: y = W2 relu(W1 x + b1) + b2
        self._k("head_fc2_bwd_w", lib.ffno_plin_bwd_weights, _p(gy), 1, None, _p(sl.H), HEAD_DIM, _p(ws.part),
                _p(gp("feedforward.2.weight")), _p(gp("feedforward.2.bias")), P, HEAD_DIM, 1, acc, 0, st)
        self._k("head_fc2_bwd", lib.ffno_plin_bwd_data, _p(gy), 1, None, _p(pp("feedforward.2.weight")), _p(ws.DH), HEAD_DIM,
                None, P, HEAD_DIM, 1, 0, 0, st)
        self._k("head_fc1_bwd_w", lib.ffno_plin_bwd_weights, _p(ws.DH), HEAD_DIM, _p(sl.H), _p(XL), C, _p(ws.part),
                _p(gp("feedforward.0.weight")), _p(gp("feedforward.0.bias")), P, C, HEAD_DIM, acc, 1, st)
        g = ws.G[0]
        self._k("head_fc1_bwd", lib.ffno_plin_bwd_data, _p(ws.DH), HEAD_DIM, _p(sl.H), _p(pp("feedforward.0.weight")), _p(g), C,
                None, P, C, HEAD_DIM, 0, 1, st)
        cur = 0
        for l in range(L - 1, -1, -1):
            pre = f"spectral_layers.{l}."
            xin = sl.X[l]
            act = sl.A[l] if self.residual else sl.X[l + 1]       # the ReLU output of this layer
            gn = ws.G[1 - cur]
            res = g if self.residual else None                    # x = layer(x) + x: g also flows straight through
            lin_in = xin if self.conv_residual else sl.S[l]
            self._k("layer_linear_bwd_w", lib.ffno_plin_bwd_weights, _p(g), C, _p(act), _p(lin_in), C, _p(ws.part),
                    _p(gp(pre + "linear.weight")), _p(gp(pre + "linear.bias")), P, C, C, acc, 1, st)
            if self.conv_residual:
                # dpre = g * 1[out > 0] feeds both the linear (here) and the spectral adjoint (below)
                self._k("layer_linear_bwd", lib.ffno_plin_bwd_data, _p(g), C, _p(act), _p(pp(pre + "linear.weight")), _p(gn),
                        C, _p(ws.DP), P, C, C, 0, 1, st)
                ws.chain.conv(ws.DP, gn, ws.SD, ws.SY, self.planes[l][1], ws.scr, False, st, resid=res, accumulate=1)
            else:
                self._k("layer_linear_bwd", lib.ffno_plin_bwd_data, _p(g), C, _p(act), _p(pp(pre + "linear.weight")),
                        _p(ws.DP), C, None, P, C, C, 0, 1, st)
                ws.chain.conv(ws.DP, gn, ws.SD, ws.SY, self.planes[l][1], ws.scr, False, st, resid=res)
            ws.chain.fw_grad_partial(sl.SX[l], ws.SD, ws.fwpart, st)
            self._k("fw2d_grad_reduce", lib.ffno_fw2d_grad_reduce, _p(ws.fwpart), _p(gp(pre + "fourier_weight.0")),
                    _p(gp(pre + "fourier_weight.1")), C, self.K, 1, acc, st)
            g, cur = gn, 1 - cur
        self._k("in_proj_bwd_w", lib.ffno_plin_bwd_weights, _p(g), C, None, _p(sl.x), Cin, _p(ws.part),
                _p(gp("in_proj.weight")), _p(gp("in_proj.bias")), P, Cin, C, acc, 0, st)
        dx = None
        if need_dx:
            dx = torch.empty(P, Cin, dtype=torch.float32, device=self.device)
            self._k("in_proj_bwd", lib.ffno_plin_bwd_data, _p(g), C, None, _p(pp("in_proj.weight")), _p(dx), Cin, None, P, Cin,
                    C, 0, 0, st)
            dx = dx.view(B, M, N, Cin)
        if self._n_pad:
            self._k("pad_copy(grads)", lib.ffno_pad_copy, _p(self._gtab), self._n_pad, 0, st)
        return (self.gflat, dx) if need_dx else self.gflat
