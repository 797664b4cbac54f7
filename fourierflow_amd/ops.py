"""Operator-level autograd wrappers over the C ABI (include/ffno.h).

These expose the single operators of the hot path the way the reference exposes them as module
methods (``SpectralConv2d.forward_fourier``, ``FeedForward.forward``); the whole-block fast path is
:class:`fourierflow_amd.engine.FFNO2DEngine`.  HIP only -- CPU tensors raise.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _capi, _lib
from ._corner_chain import CornerChain, checked
from ._lib import ptr as _p
from .engine import MODES


_SP2D_WS = {}
_SP2D_SRC = {}      # workspace key -> (weakref of the two weight tensors a version was declared for, generation)
_SP2D_GEN = [0]


def _spectral2d_workspace(x, w_y, w_x, modes):
    """The operator's workspace for a shape, kept per (shape, device): besides the scratch spectra it holds the packed weight sets
    of the fused kernels (ffno_spectral2d_path), and the library reuses them across calls when the caller declares the VERSION of
    the weights (include/ffno.h: ffno_spectral2d_weights_version) -- here (data pointer, torch version counter) of both tensors, so
    a forward / backward pair and repeated calls on unchanged weights pack once, and an optimizer step re-packs.  A tensor that
    was freed can hand its address AND its version count to a new one (the caching allocator reuses blocks; a fresh parameter starts
    at the same small count), so the declared version also carries a generation that advances whenever the weight OBJECTS differ
    from the ones the last version was declared for."""
    import weakref
    lib = _lib.get_lib()
    B, M, N, C = x.shape
    key = (B, M, N, C, modes, str(x.device), _lib.is_test_backend())
    ws = _SP2D_WS.get(key)
    if ws is None:
        ws = torch.empty(int(lib.ffno_spectral2d_ws_floats(B, M, N, C, modes)), dtype=torch.float32, device=x.device)
        _SP2D_WS[key] = ws
        while len(_SP2D_WS) > 8:
            _SP2D_WS.pop(next(iter(_SP2D_WS)))
    version = 0
    if w_y is not None and w_x is not None:
        try:
            src = _SP2D_SRC.get(key)
            if src is None or src[0]() is not w_y or src[1]() is not w_x:
                _SP2D_GEN[0] += 1
                src = _SP2D_SRC[key] = (weakref.ref(w_y), weakref.ref(w_x), _SP2D_GEN[0])
                for k in [k for k in _SP2D_SRC if k not in _SP2D_WS]:
                    del _SP2D_SRC[k]
            version = (hash((w_y.data_ptr(), w_y._version, w_x.data_ptr(), w_x._version, src[2])) & 0x7FFFFFFFFFFFFFFF) or 1
        except RuntimeError:        # inference tensors have no version counter: undeclared, the library packs on every call
            version = 0
    _capi.check(lib.ffno_spectral2d_weights_version(_p(ws), version), "spectral2d_weights_version")
    return ws


class _SpectralConv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_y, w_x, modes, mode_id):
        lib = _lib.get_lib()
        B, M, N, C = x.shape
        st = _lib.current_stream(x.device)
        ws = _spectral2d_workspace(x, w_y, w_x, modes)
        out = torch.empty_like(x)
        twn, twm = _lib.twiddle(N, x.device), _lib.twiddle(M, x.device)
        _capi.check(lib.ffno_spectral2d_fwd(_p(x), _p(w_y), _p(w_x), _p(out), _p(ws), _p(twn), _p(twm), B, M, N, C,
                                            modes, mode_id, st), "spectral2d_fwd")
        ctx.save_for_backward(x, w_y, w_x)
        ctx.cfg = (modes, mode_id)
        return out

    @staticmethod
    def backward(ctx, gy):
        x, w_y, w_x = ctx.saved_tensors
        modes, mode_id = ctx.cfg
        lib = _lib.get_lib()
        B, M, N, C = x.shape
        st = _lib.current_stream(x.device)
        gy = gy.contiguous()
        ws = _spectral2d_workspace(x, w_y, w_x, modes)
        gx = torch.empty_like(x)
        full = mode_id == MODES["full"]
        gwy = torch.empty_like(w_y) if full else None
        gwx = torch.empty_like(w_x) if full else None
        twn, twm = _lib.twiddle(N, x.device), _lib.twiddle(M, x.device)
        _capi.check(lib.ffno_spectral2d_bwd(_p(x), _p(w_y), _p(w_x), _p(gy), _p(gx), _p(gwy), _p(gwx), _p(ws), _p(twn),
                                            _p(twm), B, M, N, C, modes, mode_id, 0, 0, st), "spectral2d_bwd")
        return gx, gwy, gwx, None, None


def spectral_conv2d(x, w_y, w_x, modes: int, mode: str = "full"):
    """``SpectralConv2d.forward_fourier`` (reference grid_2d.py:51-99): x [B,M,N,C] -> [B,M,N,C].
    ``w_y`` = fourier_weight[0] (last spatial axis), ``w_x`` = fourier_weight[1]."""
    _lib.require_device_tensor(x, "spectral_conv2d input")
    if mode not in ("full", "low-pass"):
        raise ValueError("mode must be 'full' or 'low-pass'")
    B, M, N, C = x.shape
    if modes > N // 2 + 1 or modes > M // 2 + 1:
        raise ValueError(f"modes={modes} exceeds grid//2+1 for grid {M}x{N}")
    return _SpectralConv2dFn.apply(x.contiguous(), w_y.contiguous(), w_x.contiguous(), modes, MODES[mode])


class _WeightNormFn(torch.autograd.Function):
    @staticmethod
    def _run(g, v, w, dw, dg, dv, bwd):
        lib = _lib.get_lib()
        desc = _capi.WnDesc(g.data_ptr(), v.data_ptr(), w.data_ptr() if w is not None else 0,
                            dw.data_ptr() if dw is not None else 0,
                            dg.data_ptr() if dg is not None else 0,
                            dv.data_ptr() if dv is not None else 0, v.shape[0], v.shape[1])
        dev = _lib.device_table(_capi.WnDesc, [desc], v.device)
        fn = lib.ffno_weightnorm_bwd if bwd else lib.ffno_weightnorm_fwd
        _capi.check(fn(_p(dev), 1, v.shape[0], _lib.current_stream(v.device)), "weightnorm")
        return dev  # keep alive until enqueued work is ordered behind later work on the same stream

    @staticmethod
    def forward(ctx, g, v):
        w = torch.empty_like(v)
        ctx.keep = _WeightNormFn._run(g, v, w, None, None, None, False)
        ctx.save_for_backward(g, v)
        return w

    @staticmethod
    def backward(ctx, dw):
        g, v = ctx.saved_tensors
        dw = dw.contiguous()
        dg, dv = torch.empty_like(g), torch.empty_like(v)
        ctx.keep2 = _WeightNormFn._run(g, v, None, dw, dg, dv, True)
        return dg, dv


def weight_norm_weight(lin) -> torch.Tensor:
    """Effective weight of a WNLinear container (W = g v/||v||, linear.py:48-49) through the HIP kernel."""
    if not lin.wnorm:
        return lin.weight
    return _WeightNormFn.apply(lin.weight_g.contiguous(), lin.weight_v.contiguous())


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on [P, Cin] rows through the pointwise-linear kernels (csrc/plin.hip)."""

    @staticmethod
    def forward(ctx, x, W, b):
        lib = _lib.get_lib()
        P, Cin, Cout = x.shape[0], x.shape[1], W.shape[0]
        out = torch.empty(P, Cout, dtype=torch.float32, device=x.device)
        _capi.check(lib.ffno_plin_fwd(_p(x), Cin, _p(W), _p(b), None, _p(out), Cout, None, None, None, P, Cin, Cout, 0,
                                      _lib.current_stream(x.device)), "plin_fwd")
        ctx.save_for_backward(x, W)
        return out

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        lib = _lib.get_lib()
        P, Cin, Cout = x.shape[0], x.shape[1], W.shape[0]
        st = _lib.current_stream(x.device)
        g = g.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _capi.check(lib.ffno_plin_bwd_data(_p(g), Cout, None, _p(W), _p(dx), Cin, None, P, Cin, Cout, 0, 0, st), "plin_bwd_data")
        part = torch.empty(int(lib.ffno_plin_wgrad_partial_floats(P, Cin, Cout)), dtype=torch.float32, device=x.device)
        dW, db = torch.empty_like(W), torch.empty(Cout, dtype=torch.float32, device=x.device)
        _capi.check(lib.ffno_plin_bwd_weights(_p(g), Cout, None, _p(x), Cin, _p(part), _p(dW), _p(db), P, Cin, Cout, 0, 0, st),
                    "plin_bwd_weights")
        return dx, dW, db


@functools.lru_cache(maxsize=32)
def _zero_bias(n, device):
    """The bias of a linear without one: the C ABI documents no null bias for ffno_plin_fwd.  Read only, so one per (n, device)."""
    with torch.inference_mode(False):
        return torch.zeros(n, dtype=torch.float32, device=device)


def linear(rows, W, b=None):
    """y = rows W^T + b: rows [P, Cin], W [Cout, Cin], b [Cout] or None -> [P, Cout].  Differentiable in all three."""
    _lib.require_device_tensor(rows, "linear input")
    if rows.dim() != 2 or W.dim() != 2 or rows.shape[1] != W.shape[1]:
        raise ValueError(f"expected rows [P, Cin] and W [Cout, Cin], got {tuple(rows.shape)} and {tuple(W.shape)}")
    if not _lib.get_lib().ffno_plin_supported(W.shape[1], W.shape[0]):
        raise ValueError(f"linear {W.shape[1]} -> {W.shape[0]} is outside the pointwise-linear kernel set (both widths <= 128)")
    return _LinearFn.apply(rows.contiguous(), W.contiguous(), _zero_bias(W.shape[0], rows.device) if b is None else b)


def wn_linear(x, lin):
    """``WNLinear.forward`` (reference linear.py:41-52 = nn.Linear with weight_norm): x [..., in] -> [..., out]."""
    _lib.require_device_tensor(x, "WNLinear input")
    if x.shape[-1] != lin.in_features:
        raise ValueError(f"expected {lin.in_features} input features, got {tuple(x.shape)}")
    if not _lib.get_lib().ffno_plin_supported(lin.in_features, lin.out_features):
        raise NotImplementedError(f"stand-alone WNLinear({lin.in_features}, {lin.out_features}) is outside the pointwise-linear "
                                  "kernel set (both widths <= 128); inside the F-FNO block the linears run in the fused kernels")
    y = linear(x.reshape(-1, lin.in_features), weight_norm_weight(lin), lin.bias)
    return y.view(*x.shape[:-1], lin.out_features)


class _FeedForwardFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, resid, W1, b1, W2, b2):
        lib = _lib.get_lib()
        P, C, H = s.shape[0], s.shape[1], W1.shape[0]
        st = _lib.current_stream(s.device)
        out = torch.empty_like(s)
        need = any(ctx.needs_input_grad)
        h = torch.empty(P, H, dtype=torch.float32, device=s.device) if need else None
        mask = torch.zeros(int(lib.ffno_ff_mask_words(P, H)), dtype=torch.int32, device=s.device) if need else None
        _capi.check(lib.ffno_ff_fwd(_p(s), _p(resid), _p(W1), _p(b1), _p(W2), _p(b2), _p(out), _p(h), _p(mask), P, C, H, st),
                    "ff_fwd")
        ctx.save_for_backward(s, W1, W2, h, mask)
        ctx.has_resid = resid is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        s, W1, W2, h, mask = ctx.saved_tensors
        lib = _lib.get_lib()
        P, C, H = s.shape[0], s.shape[1], W1.shape[0]
        st = _lib.current_stream(s.device)
        gout = gout.contiguous()
        dh = torch.empty(P, H, dtype=torch.float32, device=s.device)
        ds = torch.empty_like(s)
        W1t, W2t = W1.t().contiguous(), W2.t().contiguous()
        _capi.check(lib.ffno_ff_bwd_data(_p(gout), _p(mask), _p(W1t), _p(W2t), _p(dh), _p(ds), P, C, H, st), "ff_bwd_data")
        nsplit = max(1, min(256, (P + 127) // 128))
        part = torch.empty(int(lib.ffno_ff_wgrad_partial_floats(C, H, nsplit)), dtype=torch.float32, device=s.device)
        _capi.check(lib.ffno_ff_bwd_weights_partial(_p(s), _p(gout), _p(h), _p(dh), _p(part), P, C, H, nsplit, st),
                    "ff_bwd_weights_partial")
        dW1, dW2 = torch.empty_like(W1), torch.empty_like(W2)
        db1 = torch.empty(H, dtype=torch.float32, device=s.device)
        db2 = torch.empty(C, dtype=torch.float32, device=s.device)
        _capi.check(lib.ffno_ff_bwd_weights_reduce(_p(part), _p(dW1), _p(dW2), _p(db1), _p(db2), C, H, nsplit, 0, st),
                    "ff_bwd_weights_reduce")
        return ds, (gout if ctx.has_resid else None), dW1, db1, dW2, db2


def feedforward(x, resid, lin0, lin1):
    """``FeedForward.forward`` (feedforward.py:13-19) [+ residual]: x [..., C] -> [..., C]."""
    _lib.require_device_tensor(x, "feedforward input")
    shp = x.shape
    s = x.reshape(-1, shp[-1]).contiguous()
    r = resid.reshape(-1, shp[-1]).contiguous() if resid is not None else None
    W1, W2 = weight_norm_weight(lin0), weight_norm_weight(lin1)
    out = _FeedForwardFn.apply(s, r, W1.contiguous(), lin0.bias, W2.contiguous(), lin1.bias)
    return out.view(shp)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, gamma, beta, eps):
        lib = _lib.get_lib()
        P, C = t.shape
        out = torch.empty_like(t)
        stats = torch.empty(P, 2, dtype=torch.float32, device=t.device)
        _capi.check(lib.ffno_layernorm_fwd(_p(t), _p(gamma), _p(beta), None, _p(out), _p(stats), P, C, float(eps),
                                           _lib.current_stream(t.device)), "layernorm_fwd")
        ctx.save_for_backward(t, gamma, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        t, gamma, stats = ctx.saved_tensors
        lib = _lib.get_lib()
        P, C = t.shape
        g = g.contiguous()
        dt = torch.empty_like(t)
        part = torch.empty(2 * C * int(lib.ffno_layernorm_nsplit(P)), dtype=torch.float32, device=t.device)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        _capi.check(lib.ffno_layernorm_bwd(_p(t), _p(stats), _p(gamma), _p(g), None, None, _p(dt), _p(part), _p(dgamma),
                                           _p(dbeta), P, C, 0, _lib.current_stream(t.device)), "layernorm_bwd")
        return dt, dgamma, dbeta, None


def layer_norm(x, ln):
    """``nn.LayerNorm(C)`` over the last axis (the final stage of FeedForward(layer_norm=True), feedforward.py:18-19)."""
    _lib.require_device_tensor(x, "layer_norm input")
    C = x.shape[-1]
    y = _LayerNormFn.apply(x.reshape(-1, C).contiguous(), ln.weight.contiguous(), ln.bias.contiguous(), ln.eps)
    return y.view(x.shape)


class _LpRelLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        lib = _lib.get_lib()
        B = pred.shape[0]
        n = pred.numel() // B
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        g = torch.empty_like(pred)
        tmp = torch.empty(int(lib.ffno_lploss_tmp_floats(B, n)), dtype=torch.float32, device=pred.device)
        _capi.check(lib.ffno_lploss_fwd_bwd(_p(pred), _p(target), _p(loss), _p(g), _p(tmp), B, n, 1.0, None,
                                            _lib.current_stream(pred.device)), "lploss")
        ctx.save_for_backward(g)
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return g * gout, None


def lp_rel_loss(pred, target):
    """``LpLoss(size_average=True)(pred.reshape(B, -1), target.reshape(B, -1))`` (reference modules/loss.py:33-46):
    mean_b ||pred_b - target_b||_2 / ||target_b||_2, loss and gradient from one fused HIP pass."""
    _lib.require_device_tensor(pred, "pred")
    _lib.require_device_tensor(target, "target")
    if pred.numel() != target.numel() or pred.shape[0] != target.shape[0]:
        raise ValueError(f"shape mismatch: {tuple(pred.shape)} vs {tuple(target.shape)}")
    return _LpRelLossFn.apply(pred.contiguous(), target.contiguous())


def _complex64(t, ndim, what, rank_error=ValueError):
    """The view_as_real twin of a complex64 tensor of rank ``ndim``; ``what`` names it and its layout in the refusal."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.complex64:
        raise TypeError(f"{what}: expected a complex64 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != ndim:
        raise rank_error(f"{what}: expected rank {ndim}, got {tuple(t.shape)}")
    return torch.view_as_real(t)


def _check_xi(xi, B, N=None):
    """xi is a device tensor [B, N, 2]; N = None: any number of points."""
    _lib.require_device_tensor(xi, "xi")
    if xi.dim() != 3 or xi.shape[0] != B or (N is not None and xi.shape[1] != N) or xi.shape[2] != 2:
        raise ValueError(f"xi: expected [B, N, 2] = [{B}, {'N' if N is None else N}, 2], got {tuple(xi.shape)}")


def _corner_modes_check(C, m1, m2):
    if not _lib.get_lib().ffno_nudft_supported(C, m1, m2):
        raise ValueError(f"non-uniform DFT: modes ({m1}, {m2}) outside the compiled set (1..16 each)")


def _axis_modes_check(C, m1, m2):
    if m1 < 1 or m2 < 1 or not _lib.get_lib().ffno_nudft_axis_supported(C, m1, m2):
        raise ValueError(f"per-axis non-uniform DFT: modes ({m1}, {m2}) outside the compiled set (1..32 each)")


class _PointTransform(NamedTuple):
    """One points <-> modes transform of the C ABI: its points -> modes and modes -> points entry points, each with the trailing
    flags this transform fixes, the real spectrum's shape after [B, C] for (m1, m2), and its name in a failed launch's message."""
    tag: str
    modes: str
    modes_flags: tuple
    points: str
    points_flags: tuple
    spec_shape: Callable

    def to_modes(self, u, xi, spec, dims, what=""):
        """spec = sum_n u E(xi); dims = (B, C, N, m1, m2)"""
        _capi.check(getattr(_lib.get_lib(), self.modes)(_p(u), _p(xi), _p(spec), *dims, *self.modes_flags,
                                                        _lib.current_stream(u.device)), self.modes[5:] + what)

    def to_points(self, spec, xi, w, out, dxi, dims, what=""):
        """out = Re sum_k spec E(xi) (when given) and dxi = its coordinate gradient weighted with w (when given)"""
        _capi.check(getattr(_lib.get_lib(), self.points)(_p(spec), _p(xi), _p(w), _p(out), _p(dxi), *dims, *self.points_flags,
                                                         _lib.current_stream(spec.device)), self.points[5:] + what)


# fft2d and its corner slicing / ifft2d with the reference's completion of the negative-k2 half: spectra [B, C, 2 m1, m2]
_FFT2D = _PointTransform("fft2d ", "ffno_nudft_modes", (0,), "ffno_nudft_points", (0, 0), lambda m1, m2: (2 * m1, m2, 2))
_IFFT2D = _PointTransform("ifft2d ", "ffno_nudft_modes", (1,), "ffno_nudft_points", (1, 0), lambda m1, m2: (2 * m1, m2, 2))
# the per-axis transforms of the fully factorised point-cloud F-FNO (csrc/ffno_pointaxis.h).  Spectra are complex64
# [B, C, m2 + m1]: the m2 modes of coordinate 0 (the y set, fourier_weight[0]) and then the m1 modes of coordinate 1 (the x set,
# fourier_weight[1]); the autograd functions work on their view_as_real twins.
_AXIS = _PointTransform("", "ffno_nudft_axis_modes", (), "ffno_nudft_axis_points", (0,), lambda m1, m2: (m1 + m2, 2))


class _PointsToModesFn(torch.autograd.Function):
    """u [B, C, N] on the points xi -> the real twin of the spectrum of transform ``tr``."""

    @staticmethod
    def forward(ctx, u, xi, tr, m1, m2):
        B, C, N = u.shape
        spec = torch.empty(B, C, *tr.spec_shape(m1, m2), dtype=torch.float32, device=u.device)
        tr.to_modes(u, xi, spec, (B, C, N, m1, m2))
        ctx.save_for_backward(u, xi)
        ctx.cfg = (tr, m1, m2)
        return spec

    @staticmethod
    def backward(ctx, gspec):
        u, xi = ctx.saved_tensors
        tr, m1, m2 = ctx.cfg
        gspec = gspec.contiguous()
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        dxi = torch.empty_like(xi) if ctx.needs_input_grad[1] else None
        if du is not None or dxi is not None:
            # the adjoint in u is the modes -> points sum without any inverse factor: du = Re sum dY E, and w = u gives dxi in
            # the same launch
            tr.to_points(gspec, xi, u, du, dxi, (*u.shape, m1, m2), f" ({tr.tag}adjoint)")
        return du, dxi, None, None, None


class _ModesToPointsFn(torch.autograd.Function):
    """The real twin of a spectrum of transform ``tr`` -> real [B, C, N] on the points xi."""

    @staticmethod
    def forward(ctx, spec, xi, tr, m1, m2):
        B, C = spec.shape[:2]
        N = xi.shape[1]
        out = torch.empty(B, C, N, dtype=torch.float32, device=spec.device)
        tr.to_points(spec, xi, None, out, None, (B, C, N, m1, m2))
        ctx.save_for_backward(spec, xi)
        ctx.cfg = (tr, m1, m2)
        return out

    @staticmethod
    def backward(ctx, gout):
        spec, xi = ctx.saved_tensors
        tr, m1, m2 = ctx.cfg
        dims = (spec.shape[0], spec.shape[1], xi.shape[1], m1, m2)
        gout = gout.contiguous()
        dspec = dxi = None
        if ctx.needs_input_grad[0]:
            dspec = torch.empty_like(spec)
            tr.to_modes(gout, xi, dspec, dims, f" ({tr.tag}adjoint)")
        if ctx.needs_input_grad[1]:
            dxi = torch.empty_like(xi)
            tr.to_points(spec, xi, gout, None, dxi, dims, f" ({tr.tag}xi gradient)")
        return dspec, dxi, None, None, None


def _check_points(u, xi):
    _lib.require_device_tensor(u, "u")
    if u.dim() != 3:
        raise ValueError(f"u: expected [B, C, N], got {tuple(u.shape)}")
    _check_xi(xi, u.shape[0], u.shape[2])


def point_fft2d(u, xi, modes1: int, modes2: int):
    """``SpectralConv2d.fft2d(u, x_in)`` of the point-cloud F-FNO followed by its corner slicing (reference
    modules/factorized_fno/point_cloud_2d.py:95-131, :54-62): u [B, C, N] on the points xi [B, N, 2] -> complex64
    [B, C, 2 modes1, modes2], rows k1 = 0..modes1-1 then -modes1..-1, columns k2 = 0..modes2-1.  Differentiable in u and xi."""
    _check_points(u, xi)
    _corner_modes_check(u.shape[1], modes1, modes2)
    return torch.view_as_complex(_PointsToModesFn.apply(u.contiguous(), xi.contiguous(), _FFT2D, int(modes1), int(modes2)))


def point_ifft2d(spec, xi):
    """``SpectralConv2d.ifft2d(spec, x_out)`` of the point-cloud F-FNO (reference point_cloud_2d.py:133-159): complex64 spec
    [B, C, 2 m1, m2] in the layout point_fft2d returns -> real [B, C, N] on the points xi [B, N, 2], including the reference's
    `flip(-1, -2).conj()` completion of the negative-k2 half exactly as it computes it.  Differentiable in spec and xi."""
    sr = _complex64(spec, 4, "spec [B, C, 2 m1, m2]")
    if spec.shape[2] % 2:
        raise ValueError(f"spec: expected [B, C, 2 m1, m2], got {tuple(spec.shape)}")
    _lib.require_device_tensor(sr, "spec")
    B, C, R, m2 = spec.shape
    _check_xi(xi, B)
    _corner_modes_check(C, R // 2, m2)
    return _ModesToPointsFn.apply(sr.contiguous(), xi.contiguous(), _IFFT2D, R // 2, m2)


def _axis_split(spec, modes2, what):
    """(m1, m2) of a spectrum [B, C, m2 + m1]; modes2 = None means modes1 = modes2."""
    K = spec.shape[2]
    if modes2 is None:
        if K % 2:
            raise ValueError(f"{what}: {K} modes do not split evenly; pass modes2")
        modes2 = K // 2
    modes2 = int(modes2)
    if not 1 <= modes2 < K:
        raise ValueError(f"{what}: modes2 = {modes2} does not split {K} modes")
    return K - modes2, modes2


def _axis_grid_guard(m1, m2, S, C):
    if m1 > S // 2 + 1 or m2 > S // 2 + 1:
        raise ValueError(f"modes ({m1}, {m2}) exceed S // 2 + 1 = {S // 2 + 1} of a {S} x {S} latent grid")
    if S > 256 or C > 256 or S * C > 8192:
        raise ValueError(f"latent grid {S} x {S} with {C} channels is outside the compiled set (S <= 256, C <= 256, S C <= 8192)")


class _AxisGridFn(torch.autograd.Function):
    """``to_grid``: the real twin of a spectrum [B, C, m2 + m1] -> channels-last grid [B, S, S, C]; otherwise the grid -> the
    spectrum.  The two kernels are each other's adjoint under the same ``c2r`` flag: 1 around the irfft (spectrum -> grid
    forward), 0 around the rfft (grid -> spectrum forward)."""

    @staticmethod
    def _run(t, S, m1, m2, to_grid, c2r, what):
        B, C = (t.shape[0], t.shape[1]) if to_grid else (t.shape[0], t.shape[3])
        out = torch.empty((B, S, S, C) if to_grid else (B, C, m1 + m2, 2), dtype=torch.float32, device=t.device)
        lib = _lib.get_lib()
        fn = lib.ffno_axis_modes_to_grid if to_grid else lib.ffno_grid_to_axis_modes
        _capi.check(fn(_p(t), _p(out), B, C, S, m1, m2, c2r, _lib.current_stream(t.device)), what)
        return out

    @staticmethod
    def forward(ctx, t, S, m1, m2, to_grid):
        ctx.cfg = (S, m1, m2, to_grid)
        return _AxisGridFn._run(t, S, m1, m2, to_grid, int(to_grid), "axis_modes_to_grid" if to_grid else "grid_to_axis_modes")

    @staticmethod
    def backward(ctx, g):
        S, m1, m2, to_grid = ctx.cfg
        what = "grid_to_axis_modes (adjoint)" if to_grid else "axis_modes_to_grid (adjoint)"
        return _AxisGridFn._run(g.contiguous(), S, m1, m2, not to_grid, int(to_grid), what), None, None, None, None


def point_axis_fft(u, xi, modes1: int, modes2: int):
    """The two "bcn,bnxy->bcxy" einsums of the fully factorised point-cloud SpectralConv2d over its one-dimensional bases
    (reference modules/factorized_fno/mesh_plus_2d.py:65, :93 with get_fft_bases :118-142): u [B, C, N] on the points xi
    [B, N, 2] -> complex64 [B, C, modes2 + modes1], sum_n u exp(-2 pi i j xi_0) for j < modes2, then sum_n u exp(-2 pi i k xi_1)
    for k < modes1.  Differentiable in u and xi."""
    _check_points(u, xi)
    _axis_modes_check(u.shape[1], int(modes1), int(modes2))
    return torch.view_as_complex(_PointsToModesFn.apply(u.contiguous(), xi.contiguous(), _AXIS, int(modes1), int(modes2)))


def point_axis_ifft(spec, xi, modes2=None):
    """The two "bcxy,bnxy->bcn" einsums over get_ifft_bases and their sum (mesh_plus_2d.py:83-84, :109-110, :114, :144-168) once
    the repeated grid axis is summed: complex64 spec [B, C, modes2 + modes1] in point_axis_fft's layout -> real [B, C, N] =
    Re sum_j spec_j exp(2 pi i j xi_0) + Re sum_k spec_{modes2 + k} exp(2 pi i k xi_1), no normalisation.  ``modes2`` = None
    means modes1 = modes2.  Differentiable in spec and xi."""
    sr = _complex64(spec, 3, "spec [B, C, modes2 + modes1]")
    m1, m2 = _axis_split(spec, modes2, "spec")
    _lib.require_device_tensor(sr, "spec")
    B, C = spec.shape[:2]
    _check_xi(xi, B)
    _axis_modes_check(C, m1, m2)
    return _ModesToPointsFn.apply(sr.contiguous(), xi.contiguous(), _AXIS, m1, m2)


def axis_modes_to_grid(spec, S: int, modes2=None):
    """The x_out = None branch of the fully factorised point-cloud SpectralConv2d after its mix (mesh_plus_2d.py:69-78, :97-106,
    :114): complex64 spec [B, C, modes2 + modes1] -> channels-last real [B, S, S, C] = h(x) + g(y), g = torch.fft.irfft of the
    first modes2 modes zero-padded to S // 2 + 1 (n = S), h likewise of the last modes1.  Differentiable in spec."""
    sr = _complex64(spec, 3, "spec [B, C, modes2 + modes1]")
    m1, m2 = _axis_split(spec, modes2, "spec")
    _lib.require_device_tensor(sr, "spec")
    _axis_modes_check(spec.shape[1], m1, m2)
    _axis_grid_guard(m1, m2, int(S), spec.shape[1])
    return _AxisGridFn.apply(sr.contiguous(), int(S), m1, m2, True)


def grid_to_axis_modes(x, modes1: int, modes2: int):
    """The x_in = None branch up to its mix when the output lies on points (mesh_plus_2d.py:61, :89 and the sum over the repeated
    basis axis of :83-84, :109-110): channels-last grid x [B, S, S, C] -> complex64 [B, C, modes2 + modes1], rfft over y of
    sum_x x truncated to modes2, then rfft over x of sum_y x truncated to modes1.  Differentiable in x."""
    _lib.require_device_tensor(x, "grid")
    if x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise ValueError(f"expected a square channels-last grid [B, S, S, C], got {tuple(x.shape)}")
    m1, m2 = int(modes1), int(modes2)
    _axis_modes_check(x.shape[3], m1, m2)
    _axis_grid_guard(m1, m2, x.shape[1], x.shape[3])
    return torch.view_as_complex(_AxisGridFn.apply(x.contiguous(), x.shape[1], m1, m2, False))


# ---- grid <-> corner modes: the two ends of the point-cloud F-FNO's latent grid (rfft2 / irfft2 restricted to the kept corners) ----
# Mode-major spectra are the grid kernels' layout: Z[ky][kx'][b][re/im][c], kx' < m1 the rows k1 = kx', kx' >= m1 the rows
# k1 = kx' - 2 m1; the non-uniform DFT's layout is [b][c][kx'][ky][re/im].  The kernels' twiddle tables carry 1 / sqrt(L) per
# axis (norm='ortho'), so torch's default normalisations (1 for rfft2, 1 / (s1 s2) for irfft2) are a factor sqrt(s1 s2) away.

def _corner_guard(m1, m2, s1, s2, C):
    if m1 < 1 or m2 < 1 or 2 * m1 > s1 or m2 > s2 // 2 or m1 > min(s1, s2) // 2 + 1:
        raise ValueError(f"modes ({m1}, {m2}) do not fit a {s1} x {s2} latent grid (need 2 modes1 <= s1, modes2 <= s2 // 2, "
                         f"modes1 <= min(s1, s2) // 2 + 1)")
    if C not in (32, 64):
        raise ValueError(f"width {C} is outside the compiled channel tiles (32 / 64)")


def _modes_major(spec_r):
    """[B, C, 2 m1, m2, 2] -> [m2, 2 m1, B, 2, C]"""
    return spec_r.permute(3, 2, 0, 4, 1)


def _points_major(z):
    """[m2, 2 m1, B, 2, C] -> [B, C, 2 m1, m2, 2]"""
    return z.permute(2, 4, 1, 0, 3)


@functools.lru_cache(maxsize=32)
def _chain(B, Sp, Ks, C, device, emu) -> CornerChain:
    """The chain of a shape and backend (geometry and table pointers only, so it is kept across calls)."""
    return CornerChain(B, Sp, Ks, C, checked, device)


def _scratch(ch):
    """Per-call scratch of one half of the chain: the spectra between its stages and the row-transform scratch."""
    f32 = dict(dtype=torch.float32, device=ch.device)
    return [torch.empty(n, **f32) for n in ch.mid_sizes], torch.empty(ch.cw_floats, **f32)


class _ModesToGridFn(torch.autograd.Function):
    """Z [m2, 2 m1, B, 2, C] (mode-major corners) -> channels-last grid [B, s1, s2, C] = irfft2 of the zero-padded spectrum."""

    @staticmethod
    def forward(ctx, z, s1, s2):
        m2, R, B, _, C = z.shape
        ctx.chain = ch = _chain(B, (s1, s2), (R // 2, m2), C, z.device, _lib.is_test_backend())
        zs = (z * (1.0 / float(np.sqrt(s1 * s2)))).contiguous()
        out = torch.empty(B, s1, s2, C, dtype=torch.float32, device=z.device)
        mid, cw = _scratch(ch)
        ch.synthesis(zs, mid, out, cw, True, _lib.current_stream(z.device))
        return out

    @staticmethod
    def backward(ctx, g):
        ch = ctx.chain
        g = g.contiguous()
        dz = torch.empty(ch.Ks[1], 2 * ch.Ks[0], ch.B, 2, ch.C, dtype=torch.float32, device=g.device)
        mid, cw = _scratch(ch)
        # the adjoint of the zero-padded irfft (bins k >= 1 counted twice), then the adjoint of the inverse row transform
        ch.analysis(g, mid, dz, cw, False, _lib.current_stream(g.device))
        return dz * (1.0 / float(np.sqrt(ch.Sp[0] * ch.Sp[1]))), None, None


def _pack_corner_weights(ch, w1, w2, st):
    """The two corner weight tensors ([C, C, m1, m2, 2] each) packed for ch.mix -> (the set of the forward mix `bixy,ioxy->boxy`,
    the transposed set of its adjoint)."""
    f32 = dict(dtype=torch.float32, device=w1.device)
    wp, wpt = torch.empty(ch.planes_floats, **f32), torch.empty(ch.planes_floats, **f32)
    _capi.check(_lib.get_lib().ffno_fw2d_pack2(_p(w1), _p(w2), _p(wp), _p(wpt), ch.C, *ch.Ks, st), "fw2d_pack2")
    return wp, wpt


def _corner_weight_grads(ch, z, dy, st):
    """The gradients of the two corner weight tensors from the mix's input z and output gradient dy: per-workgroup partial sums,
    then one fixed-order reduction."""
    f32 = dict(dtype=torch.float32, device=dy.device)
    (m1, m2), C = ch.Ks, ch.C
    part = torch.empty(ch.planes_floats, **f32)
    gw1, gw2 = torch.empty(C, C, m1, m2, 2, **f32), torch.empty(C, C, m1, m2, 2, **f32)
    ch.fw_grad_partial(z, dy, part, st)
    _capi.check(_lib.get_lib().ffno_fw2d_grad_reduce2(_p(part), _p(gw1), _p(gw2), C, m1, m2, 1, 0, st), "fw2d_grad_reduce2")
    return gw1, gw2


class _GridToMixedModesFn(torch.autograd.Function):
    """Channels-last grid [B, s1, s2, C] -> mode-major corners of rfft2 mixed with the two corner weight tensors
    ([C, C, m1, m2, 2] each, `bixy,ioxy->boxy`): [m2, 2 m1, B, 2, C]."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        B, s1, s2, C = x.shape
        m1, m2 = w1.shape[2], w1.shape[3]
        ctx.chain = ch = _chain(B, (s1, s2), (m1, m2), C, x.device, _lib.is_test_backend())
        st = _lib.current_stream(x.device)
        f32 = dict(dtype=torch.float32, device=x.device)
        wp, wpt = _pack_corner_weights(ch, w1, w2, st)
        mid, cw = _scratch(ch)
        sx, out = torch.empty(ch.spec, **f32), torch.empty(m2, 2 * m1, B, 2, C, **f32)
        ch.analysis(x, mid, sx, cw, True, st)
        ch.mix(sx, wp, out, True, st)
        ctx.save_for_backward(sx, wpt)
        return out * float(np.sqrt(s1 * s2))

    @staticmethod
    def backward(ctx, g):
        sx, wpt = ctx.saved_tensors
        ch = ctx.chain
        (s1, s2), B, C = ch.Sp, ch.B, ch.C
        st = _lib.current_stream(g.device)
        f32 = dict(dtype=torch.float32, device=g.device)
        dy = (g * float(np.sqrt(s1 * s2))).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dsx = torch.empty(ch.spec, **f32)
            mid, cw = _scratch(ch)
            dx = torch.empty(B, s1, s2, C, **f32)
            ch.mix(dy, wpt, dsx, False, st)
            ch.synthesis(dsx, mid, dx, cw, False, st)
        return (dx, *_corner_weight_grads(ch, sx, dy, st))


def modes_to_grid(z, s1: int, s2: int):
    """Mode-major corners [m2, 2 m1, B, 2, C] -> [B, s1, s2, C] (see corners_to_grid)."""
    _lib.require_device_tensor(z, "corner modes")
    if z.dim() != 5 or z.shape[1] % 2 or z.shape[3] != 2:
        raise ValueError(f"expected mode-major corners [m2, 2 m1, B, 2, C], got {tuple(z.shape)}")
    _corner_guard(z.shape[1] // 2, z.shape[0], s1, s2, z.shape[4])
    return _ModesToGridFn.apply(z, int(s1), int(s2))


def corners_to_grid(spec, s1: int, s2: int):
    """The x_out = None branch of the point-cloud SpectralConv2d (reference point_cloud_2d.py:70-74): complex64 corners
    [B, C, 2 modes1, modes2] in point_fft2d's layout are placed in rows [0, m1) and [s1 - m1, s1), columns [0, m2) of an
    s1 x (s2 // 2 + 1) spectrum and transformed by ``torch.fft.irfft2(., s=(s1, s2))`` -> channels-last real [B, s1, s2, C]."""
    return modes_to_grid(_modes_major(_complex64(spec, 4, "spec [B, C, 2 m1, m2]", rank_error=TypeError)), s1, s2)


def grid_to_mixed_modes(x, w1, w2):
    """Channels-last grid -> mixed mode-major corners (see grid_to_mixed_corners); w1 / w2 real views [C, C, m1, m2, 2]."""
    _lib.require_device_tensor(x, "grid")
    if x.dim() != 4 or w1.shape != w2.shape or w1.dim() != 5 or w1.shape[0] != x.shape[3] or w1.shape[1] != x.shape[3]:
        raise ValueError(f"expected x [B, s1, s2, C] and two weights [C, C, m1, m2, 2], got {tuple(x.shape)}, {tuple(w1.shape)}")
    _corner_guard(w1.shape[2], w1.shape[3], x.shape[1], x.shape[2], x.shape[3])
    return _GridToMixedModesFn.apply(x.contiguous(), w1.contiguous(), w2.contiguous())


def grid_to_mixed_corners(x, weights1, weights2):
    """The x_in = None branch of the point-cloud SpectralConv2d up to the concatenation (reference point_cloud_2d.py:49, :60-63,
    :76): ``torch.fft.rfft2`` of the channels-last grid x [B, s1, s2, C], rows [:m1] mixed with weights1 and rows [-m1:] with
    weights2 (`bixy,ioxy->boxy`, columns [:m2]; complex64 [C, C, m1, m2] or their view_as_real twins), concatenated ->
    complex64 [B, C, 2 m1, m2], what point_ifft2d takes.  Differentiable in x and both weights."""
    w1 = torch.view_as_real(weights1) if weights1.is_complex() else weights1
    w2 = torch.view_as_real(weights2) if weights2.is_complex() else weights2
    return torch.view_as_complex(_points_major(grid_to_mixed_modes(x, w1, w2)).contiguous())


class _MixCornerModesFn(torch.autograd.Function):
    """Mode-major corners z [m2, 2 m1, B, 2, C] mixed with the two corner weight tensors ([C, C, m1, m2, 2] each,
    `bixy,ioxy->boxy`): the launches _GridToMixedModesFn runs after its analysis, on a spectrum the caller already has."""

    @staticmethod
    def forward(ctx, z, w1, w2, grid):
        m2, R, B, _, C = z.shape
        ctx.chain = ch = _chain(B, grid, (R // 2, m2), C, z.device, _lib.is_test_backend())
        st = _lib.current_stream(z.device)
        wp, wpt = _pack_corner_weights(ch, w1, w2, st)
        out = torch.empty_like(z)
        ch.mix(z, wp, out, True, st)
        ctx.save_for_backward(z, wpt)
        return out

    @staticmethod
    def backward(ctx, g):
        z, wpt = ctx.saved_tensors
        ch = ctx.chain
        st = _lib.current_stream(g.device)
        g = g.contiguous()
        dz = None
        if ctx.needs_input_grad[0]:
            dz = torch.empty_like(z)
            ch.mix(g, wpt, dz, False, st)
        return (dz, *_corner_weight_grads(ch, z, g, st), None)


def mix_corner_modes(z, w1, w2, grid=None):
    """The corner mix of the point-cloud SpectralConv2d on a spectrum that is already in mode space (reference
    zongyi_fno/point_cloud_2d.py:56-59 after fft2d): z [m2, 2 m1, B, 2, C] mode-major corners, rows kx' < m1 x w1 and rows
    kx' >= m1 x w2 (`bixy,ioxy->boxy`; real views [C, C, m1, m2, 2]) -> the same layout.  Differentiable in z and both weights.
    ``grid`` = (s1, s2) of the latent grid the spectrum goes to: the op then shares the chain of the neighbouring
    modes_to_grid / grid_to_mixed_modes (the mix itself does not depend on it)."""
    _lib.require_device_tensor(z, "corner modes")
    if z.dim() != 5 or z.shape[1] % 2 or z.shape[3] != 2:
        raise ValueError(f"expected mode-major corners [m2, 2 m1, B, 2, C], got {tuple(z.shape)}")
    m2, m1, C = z.shape[0], z.shape[1] // 2, z.shape[4]
    if w1.shape != w2.shape or tuple(w1.shape) != (C, C, m1, m2, 2):
        raise ValueError(f"expected two weights [{C}, {C}, {m1}, {m2}, 2], got {tuple(w1.shape)}, {tuple(w2.shape)}")
    grid = (int(grid[0]), int(grid[1])) if grid is not None else (2 * m1, 2 * max(m1, m2))
    _corner_guard(m1, m2, grid[0], grid[1], C)
    return _MixCornerModesFn.apply(z.contiguous(), w1.contiguous(), w2.contiguous(), grid)


# ---- the pointwise stage of a geo-FNO layer on the latent grid (csrc/plin.hip: ffno_plin_pos_*) --------------------------------
_GRID_TABLES = {}


def _grid_tables(s1, s2, device):
    """tx[s1], ty[s2]: the reference's grid coordinates, float32(np.linspace(0, 1, s)) (point_cloud_2d.py:245-253), and the pixel
    coordinates [s1 * s2, 2] made of them, row-major.  One entry per (s1, s2, device), read only."""
    key = (int(s1), int(s2), str(torch.device(device)))
    if key not in _GRID_TABLES:
        with torch.inference_mode(False):      # (kept across calls and saved for backward: never inference tensors)
            tx, ty = (torch.tensor(np.linspace(0, 1, s), dtype=torch.float).to(device) for s in key[:2])
            _GRID_TABLES[key] = (tx, ty, torch.cartesian_prod(tx, ty))
    return _GRID_TABLES[key]


def latent_grid(s1: int, s2: int, device):
    """The coordinates of the pixels of an s1 x s2 latent grid, row-major [s1 * s2, 2]: the reference's ``get_grid``
    (point_cloud_2d.py:272-280) flattened, from the tables above."""
    return _grid_tables(s1, s2, device)[2]


class _GeoFNOPointwiseFn(torch.autograd.Function):
    """gelu(W x + add + gw . grid + b1 [+ b2]) over a [B, s1, s2, C] grid; x = W = b2 = None: no 1x1 convolution (layer 0)."""

    @staticmethod
    def forward(ctx, add, gw, b1, x, W, b2):
        lib = _lib.get_lib()
        B, s1, s2, C = add.shape
        st = _lib.current_stream(add.device)
        tx, ty, _ = _grid_tables(s1, s2, add.device)
        b = b1 if b2 is None else b1 + b2
        out, pre = torch.empty_like(add), torch.empty_like(add)
        _capi.check(lib.ffno_plin_pos_fwd(_p(x), C, _p(W), _p(b), _p(add), _p(gw), _p(tx), _p(ty), _p(out), C, _p(pre), B, s1, s2, C,
                                          C, 2, st), "plin_pos_fwd")
        ctx.save_for_backward(pre, x, W)
        return out

    @staticmethod
    def backward(ctx, g):
        pre, x, W = ctx.saved_tensors
        lib = _lib.get_lib()
        B, s1, s2, C = pre.shape
        P = B * s1 * s2
        st = _lib.current_stream(g.device)
        tx, ty, _ = _grid_tables(s1, s2, g.device)
        g = g.contiguous()
        f32 = dict(dtype=torch.float32, device=g.device)
        dpre, dx, dW = torch.empty_like(pre), None, None
        if x is not None:
            dx, dW = torch.empty_like(x), torch.empty_like(W)
            _capi.check(lib.ffno_plin_bwd_data(_p(g), C, _p(pre), _p(W), _p(dx), C, _p(dpre), P, C, C, 0, 2, st), "plin_bwd_data")
        part = torch.empty(int(lib.ffno_plin_wgrad_nsplit(P)) * C * (C + 3), **f32)
        db, dgw = torch.empty(C, **f32), torch.empty(C, 2, **f32)
        _capi.check(lib.ffno_plin_pos_bwd_weights(_p(g), C, _p(pre), _p(x), C, _p(tx), _p(ty), _p(part), _p(dW), _p(db), _p(dgw),
                                                  None if x is not None else _p(dpre), B, s1, s2, C, C, 0, 2, st),
                    "plin_pos_bwd_weights")
        return dpre, dgw, db, dx, dW, (db if x is not None else None)


def geofno_pointwise(add, bs, x=None, ws=None):
    """The pointwise stage of a geo-FNO layer (reference zongyi_fno/point_cloud_2d.py:222-224 and :229-232):
    ``gelu(add + ws(x) + bs(grid))`` on channels-last grids [B, s1, s2, W]; ``add`` the spectral branch, bs = nn.Conv2d(2, W, 1)
    on the [0, 1]^2 coordinates of the pixels, ws = nn.Conv2d(W, W, 1) on x (both None: layer 0).  The grid term is evaluated
    inside the kernel from the two coordinate tables."""
    _lib.require_device_tensor(add, "spectral branch")
    if add.dim() != 4 or (x is None) != (ws is None) or (x is not None and x.shape != add.shape):
        raise ValueError(f"expected add [B, s1, s2, W] and x of the same shape with ws, got {tuple(add.shape)}")
    C = add.shape[3]
    if not _lib.get_lib().ffno_plin_supported(C, C):
        raise ValueError(f"width {C} is outside the pointwise-linear kernel set")
    if x is None:
        return _GeoFNOPointwiseFn.apply(add.contiguous(), bs.weight.reshape(C, 2).contiguous(), bs.bias, None, None, None)
    return _GeoFNOPointwiseFn.apply(add.contiguous(), bs.weight.reshape(C, 2).contiguous(), bs.bias, x.contiguous(),
                                    ws.weight.reshape(C, C).contiguous(), ws.bias)


# ---- the two per-point networks of the elasticity F-FNO ---------------------------------------------------------------------
def _param_struct(cls, tensors):
    return cls(*[t.data_ptr() for t in tensors])


class _IPhiFn(torch.autograd.Function):
    """xi = IPhi(x, code) (csrc/ffno_iphi.h); params in _capi.IPhiParams.NAMES order."""

    @staticmethod
    def forward(ctx, x, code, width, *params):
        lib = _lib.get_lib()
        B, N = x.shape[:2]
        need = any(ctx.needs_input_grad)
        f32 = dict(dtype=torch.float32, device=x.device)
        xi = torch.empty_like(x)
        feat = torch.empty(B * N, 4, **f32) if need else None
        acts = torch.empty(4, B * N, 4 * width, **f32) if need else None
        par = _param_struct(_capi.IPhiParams, params)
        _capi.check(lib.ffno_iphi_fwd(ctypes.byref(par), _p(x), _p(code), _p(xi), _p(feat), _p(acts), B, N, width,
                                      _lib.current_stream(x.device)), "iphi_fwd")
        if need:
            ctx.save_for_backward(x, code, feat, acts, *params)
        ctx.width = width
        return xi

    @staticmethod
    def backward(ctx, dxi):
        if ctx.needs_input_grad[0]:
            raise RuntimeError("IPhi: the gradient with respect to the input coordinates is not computed by the gfx950 kernel set "
                               "(feed it a tensor that does not require grad)")
        x, code, feat, acts, *params = ctx.saved_tensors
        lib = _lib.get_lib()
        B, N = x.shape[:2]
        width = ctx.width
        dxi = dxi.contiguous()
        grads = [torch.empty_like(p) for p in params]
        dcode = torch.empty_like(code)
        ws = torch.empty(int(lib.ffno_iphi_bwd_ws_floats(B, N, width)), dtype=torch.float32, device=x.device)
        par, gpar = _param_struct(_capi.IPhiParams, params), _param_struct(_capi.IPhiParams, grads)
        _capi.check(lib.ffno_iphi_bwd(ctypes.byref(par), ctypes.byref(gpar), _p(x), _p(code), _p(feat), _p(acts), _p(dxi),
                                      _p(dcode), _p(ws), B, N, width, _lib.current_stream(x.device)), "iphi_bwd")
        return (None, dcode if ctx.needs_input_grad[1] else None, None, *grads)


def iphi_forward(x, code, width: int, params):
    """``IPhi.forward(x, code)`` (reference modules/iphi.py:27-58): x [B, N, 2], code [B, 42] -> xi [B, N, 2]; ``params`` = the
    twelve tensors of fc0, fc_code, fc1..fc4 (weight, bias each).  Differentiable in the parameters and in code."""
    _lib.require_device_tensor(x, "IPhi input")
    _lib.require_device_tensor(code, "IPhi code")
    if x.dim() != 3 or x.shape[2] != 2 or code.dim() != 2 or code.shape[0] != x.shape[0] or code.shape[1] != 42:
        raise ValueError(f"expected x [B, N, 2] and code [B, 42], got {tuple(x.shape)} and {tuple(code.shape)}")
    if not _lib.get_lib().ffno_iphi_supported(width):
        raise ValueError(f"IPhi width {width} is outside the compiled set (16, 32, 64)")
    return _IPhiFn.apply(x.contiguous(), code.contiguous(), int(width), *[p.contiguous() for p in params])


class _PointHeadFn(torch.autograd.Function):
    """y = fc2(gelu(fc1(t + bs x + b))) on channel-major t (csrc/ffno_pchead.h)."""

    @staticmethod
    def forward(ctx, t, x, *params):
        lib = _lib.get_lib()
        B, W, N = t.shape
        O = params[4].shape[0]
        need = any(ctx.needs_input_grad)
        y = torch.empty(B, N, O, dtype=torch.float32, device=t.device)
        pre = torch.empty(B * N, 128, dtype=torch.float32, device=t.device) if need else None
        par = _param_struct(_capi.PcHeadParams, params)
        _capi.check(lib.ffno_pchead_fwd(ctypes.byref(par), _p(t), _p(x), _p(y), _p(pre), B, N, W, O, _lib.current_stream(t.device)),
                    "pchead_fwd")
        if need:
            ctx.save_for_backward(t, x, pre, *params)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.needs_input_grad[1]:
            raise RuntimeError("point head: the gradient with respect to the output coordinates is not computed by the gfx950 "
                               "kernel set (feed it a tensor that does not require grad)")
        t, x, pre, *params = ctx.saved_tensors
        lib = _lib.get_lib()
        B, W, N = t.shape
        O = params[4].shape[0]
        dy = dy.contiguous()
        grads = [torch.empty_like(p) for p in params]
        dt = torch.empty_like(t)
        part = torch.empty(int(lib.ffno_pchead_partial_floats(B, N, W, O)), dtype=torch.float32, device=t.device)
        par, gpar = _param_struct(_capi.PcHeadParams, params), _param_struct(_capi.PcHeadParams, grads)
        _capi.check(lib.ffno_pchead_bwd(ctypes.byref(par), ctypes.byref(gpar), _p(t), _p(x), _p(dy), _p(pre), _p(dt), _p(part), B, N,
                                        W, O, _lib.current_stream(t.device)), "pchead_bwd")
        return (dt, None, *grads)


def point_head(t, x_out, bs, fc1, fc2):
    """The output head of FNOFactorizedPointCloud2D (reference point_cloud_2d.py:263-270): t [B, W, N] channel-major (what
    point_ifft2d returns), x_out [B, N, 2], bs = nn.Conv1d(2, W, 1), fc1 = nn.Linear(W, 128), fc2 = nn.Linear(128, out)
    -> [B, N, out]."""
    _lib.require_device_tensor(t, "point features")
    _lib.require_device_tensor(x_out, "x_out")
    B, W, N = t.shape
    if x_out.shape != (B, N, 2):
        raise ValueError(f"x_out: expected [{B}, {N}, 2], got {tuple(x_out.shape)}")
    if not _lib.get_lib().ffno_pchead_supported(W, fc1.out_features, fc2.out_features):
        raise ValueError(f"point head (width {W}, hidden {fc1.out_features}, out {fc2.out_features}) is outside the compiled set "
                         "(width 32 / 64, hidden 128, out 1..64)")
    params = [bs.weight.reshape(W, 2), bs.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    return _PointHeadFn.apply(t.contiguous(), x_out.contiguous(), *[p.contiguous() for p in params])
