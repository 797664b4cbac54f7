"""Host driver of the WIDE F-FNO operators: widths 96 .. 256 (multiples of 32), where the tuned 32 / 64-channel kernels of
engine.py do not apply.  The reference modules are width-agnostic:

    WideFFNO2DEngine      FNOFactorized2DBlock (fourierflow/modules/factorized_fno/grid_2d.py:103-177): fourier_weight[0] mixes the
                          LAST axis, no padding, one output channel
    WideFFNOMeshEngine    FNOFactorizedMesh2D / FNOFactorizedMesh3D (mesh_2d.py:107-175, mesh_3d.py:115-189): fourier_weight[d] mixes
                          axis d, per-axis modes, the lifted features zero-padded at the end of every axis, the last backcast cropped,
                          ``output_dim`` channels

Both are one recording (WideFFNOEngine) over ONE kernel family, the batched strided fp32 GEMM of csrc/bgemm.hip (exact fp32 on
v_mfma_f32_32x32x2_f32), channels-last [B, S_0, .., S_{D-1}, C] end to end:

    lift, head          pointwise, M = pixels (of the DATA grid)
    DFT along axis d    F_d [2K x S_d] . x_line [S_d x C]; a line has row stride inner C (inner = the sizes after d), the lines are
                        batched over the inner positions (stride C) and over (b, the axes before d) (stride S_d inner C): nothing is
                        transposed, in 2-D or 3-D              (forward and inverse, and their adjoints through transposed strides)
    mode mix            [lines x 2C] . [[Wr, Wi], [-Wi, Wr]] [2C x 2C], batched over k       (adjoint: transposed strides)
    Fourier weight grad X[k]^T . dY[k], batched over k (split-K over the lines), then the fold (accumulated over layers, in a
                        fixed order, with share_weight)
    feed-forward        relu(s W1^T + b1) kept in HBM;  h W2^T + b2 + x through the residual epilogue;  backward: dh through
                        the gate epilogue, ds, and dW1, dW2 (split-K), db1, db2 (column sum).  A pass that saves nothing may run
                        the pair as ONE launch, ffno_bgemm_ff of csrc/bgemm_ff.hip (``fuse_ff``): the same bits, h stays on the CU
                        and the workspace holds no [pixels, hidden] tensor
    weight norm         the ffno_weightnorm_fwd / bwd descriptors of the main engine (they take any row length)
    pad, crop           (mesh operators) ffno_pad_embed / ffno_pad_crop of csrc/meshpad.hip between the dense lift / head and the
                        layers on the padded grid, and the same pair the other way round in the backward pass

The DFT tables are built once per (L, K) on the host in float64 and rounded to fp32: rows (re_k, im_k) interleaved, 1 / sqrt(L)
and c_k (c_0 = 1, c_k = 2) folded in, the imaginary DC row of the inverse zeroed (irfft ignores imag(Y[0])).  K <= L // 2: the
Nyquist bin is never kept.

Every pass is recorded once per (input shape, save, fused feed-forward) as a list of C calls over pre-built descriptors and
replayed.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _capi, _lib
from ._engine_core import EngineCore

_p = _lib.ptr
HEAD_DIM = 128
WIDE_WIDTHS = tuple(range(96, 257, 32))
MAX_HIDDEN = 1024
MAX_MODES = 64
# Whether a forward-only pass runs the fused feed-forward launch by default, per MEASURED width (profiles/wide_infer.md: true only
# where the fused median forward time is below the pair's by more than the larger of the two spreads, in the block AND the mesh
# presets).  A width that was not measured follows the nearest measured one.
FUSE_FF_MEASURED = {96: True, 128: True}


def fuse_ff_default(width: int) -> bool:
    return FUSE_FF_MEASURED[min(FUSE_FF_MEASURED, key=lambda w: (abs(w - width), w))]


def wide_supported(width: int) -> bool:
    """The widths this engine is built for (the 32 / 64-channel kernel set of engine.py takes 32 and 64)."""
    return width in WIDE_WIDTHS


def dft_tables(L: int, K: int):
    """(F [2K, L], Finv [L, 2K]) of rfft / irfft(norm='ortho') truncated to the K lowest bins, float64 -> fp32."""
    n = np.arange(L, dtype=np.float64)
    k = np.arange(K, dtype=np.float64)
    th = 2.0 * np.pi * np.outer(k, n) / L
    F = np.empty((2 * K, L))
    F[0::2], F[1::2] = np.cos(th) / np.sqrt(L), -np.sin(th) / np.sqrt(L)
    ck = np.where(k == 0, 1.0, 2.0)[:, None]
    Fi = np.empty((2 * K, L))
    Fi[0::2], Fi[1::2] = ck * np.cos(th) / np.sqrt(L), -ck * np.sin(th) / np.sqrt(L)
    Fi[1] = 0.0          # C2R: imag(Y[0]) is ignored
    return F.astype(np.float32), np.ascontiguousarray(Fi.T).astype(np.float32)


class _Lin:
    def __init__(self, prefix, rows, cols, wnorm):
        self.prefix, self.rows, self.cols, self.wnorm = prefix, rows, cols, wnorm
        self.weff = self.gweff = None


def _prod(v) -> int:
    return int(np.prod(v, dtype=np.int64)) if len(v) else 1


class WideFFNOEngine(EngineCore):
    """The recording both wide engines share.  ``axis_of_weight[w]``: the spatial axis fourier_weight[w] mixes; ``padding``: zeros
    appended to every spatial axis between the lift and the first layer (0: the lift writes layer 0's input and the head reads the
    last backcast directly, no copy)."""

    can_return_view = True

    def __init__(self, *, modes, width: int, input_dim: int, n_layers: int, factor: int, share_weight: bool,
                 share_fork: bool = False, ff_weight_norm: bool = False, mode: str = "full", use_fork: bool = False,
                 layer_norm: bool = False, n_ff_layers: int = 2, dropout: float = 0.0, in_dropout: float = 0.0,
                 storage=None, axis_of_weight=(1, 0), padding: int = 0, output_dim: int = 1):
        if not wide_supported(width):
            raise ValueError(f"width={width} is outside the wide engine's set {WIDE_WIDTHS}")
        C, H = width, factor * width
        narrow = "widths 32 / 64 support it"

        def refuse(option):
            raise NotImplementedError(f"{option} is not built for width {width} (the wide GEMM engine); {narrow}")
        if H > MAX_HIDDEN or factor < 1:
            raise NotImplementedError(f"factor * width = {H} > {MAX_HIDDEN} is not built for the wide GEMM engine")
        if use_fork:
            refuse("use_fork=True")
        if share_fork:
            refuse("share_fork=True")
        if layer_norm:
            refuse("layer_norm=True")
        if dropout or in_dropout:
            refuse("dropout / in_dropout > 0")
        if mode != "full":
            refuse(f"mode={mode!r}")
        if n_ff_layers != 2:
            refuse(f"n_ff_layers={n_ff_layers}")
        storage = os.environ.get("FFNO_STORAGE", "fp32") if storage is None else storage      # 
        if storage != "fp32":
            refuse(f"storage={storage!r}")
        if not (0 < input_dim):
            raise ValueError("input_dim must be positive")
        self.axis_of_weight: Tuple[int, ...] = tuple(axis_of_weight)
        self.nd = nd = len(self.axis_of_weight)
        if nd not in (2, 3) or sorted(self.axis_of_weight) != list(range(nd)):
            raise ValueError("2 or 3 spatial axes, one Fourier weight each")
        # per Fourier WEIGHT (the grid block: (K_y, K_x))
        self.Ks: Tuple[int, ...] = tuple(int(k) for k in modes) if isinstance(modes, (tuple, list)) else (int(modes),) * nd
        if len(self.Ks) != nd or not all(1 <= k <= MAX_MODES for k in self.Ks):
            raise ValueError(f"modes must be 1 .. {MAX_MODES} per axis, got {modes}")
        if padding < 0 or output_dim < 1:
            raise ValueError("padding must be >= 0 and output_dim >= 1")
        self.pad, self.O = int(padding), int(output_dim)
        self.C, self.H, self.Cin, self.L = C, H, input_dim, n_layers
        self.share_weight, self.wnorm = bool(share_weight), bool(ff_weight_norm)
        # forward(save_for_backward=False) records one ffno_bgemm_ff per layer in place of wide_ff1 + wide_ff2; read when a pass
        # is recorded (a pass recorded under the other value stays what it is)
        self.fuse_ff = fuse_ff_default(width)

        # parameter inventory: the registration order of FFNOEngine (engine.py), reference named_parameters() names
        self.linears: Dict[str, _Lin] = {}
        shapes: Dict[str, Tuple[int, ...]] = {}

        def add_linear(prefix, rows, cols):
            self.linears[prefix] = _Lin(prefix, rows, cols, self.wnorm)
            if self.wnorm:
                shapes[prefix + "weight_g"] = (rows, 1)
                shapes[prefix + "weight_v"] = (rows, cols)
            else:
                shapes[prefix + "weight"] = (rows, cols)
            shapes[prefix + "bias"] = (rows,)

        add_linear("in_proj.", C, input_dim)
        self.ff_prefix: List[str] = []
        self.fw_names: List[Tuple[str, ...]] = []
        for l in range(n_layers):
            fp = f"spectral_layers.{l}.backcast_ff."
            self.ff_prefix.append(fp)
            add_linear(fp + "layers.0.0.", H, C)
            add_linear(fp + "layers.1.0.", C, H)
            base = "fourier_weight." if share_weight else f"spectral_layers.{l}.fourier_weight."
            names = tuple(base + str(w) for w in range(nd))
            self.fw_names.append(names)
            for w, n in enumerate(names):
                shapes.setdefault(n, (C, C, self.Ks[w], 2))
        add_linear("out.0.", HEAD_DIM, C)
        add_linear("out.1.", self.O, HEAD_DIM)
        self._lay_out(shapes)
        self._fw_sets: List[Tuple[str, ...]] = list(dict.fromkeys(self.fw_names))
        self._fw_set_of = [self._fw_sets.index(n) for n in self.fw_names]

        self.params: Dict[str, torch.Tensor] = {}
        self.device = None
        self.timer = None
        self._issue_stream = 0
        self._ws = {}
        self._bind_sig = None
        self._derived_sig = None
        self._dirty = True
        self._saved = None
        self._tables = {}
        self.dx = None

    # ------------------------------------------------------------------------------------------------
    def bind(self, params: Dict[str, torch.Tensor]):
        """Attach the parameter tensors (unique reference names -> fp32 contiguous device tensors)."""
        sig = tuple(params[n].data_ptr() for n in self.param_names) if all(n in params for n in self.param_names) else None
        if sig is not None and self.params and sig == self._bind_sig:
            self.params = {n: params[n] for n in self.param_names}
            return
        dev = self._validate(params)
        self.params = {n: params[n] for n in self.param_names}
        self._bind_sig = sig
        self._dirty = True
        self._ws = {}                 # the recorded passes hold parameter addresses
        if dev != self.device:
            self.device = dev
            self._tables = {}
        f32 = dict(dtype=torch.float32, device=dev)
        C = self.C
        self.gflat = torch.zeros(self.n_params, **f32)
        n_eff = sum(l.rows * l.cols for l in self.linears.values()) if self.wnorm else 0
        self.weff_flat = torch.empty(max(n_eff, 1), **f32)
        self.gweff_flat = torch.zeros(max(n_eff, 1), **f32)
        # packed per-mode block matrices of every Fourier weight set: packs[set][axis] [K][2C][2C]
        self.packs = [[torch.empty(K, 2 * C, 2 * C, **f32) for K in self.Ks] for _ in self._fw_sets]
        off, descs = 0, []
        for lin in self.linears.values():
            n = lin.rows * lin.cols
            if lin.wnorm:
                lin.weff = self.weff_flat[off:off + n].view(lin.rows, lin.cols)
                lin.gweff = self.gweff_flat[off:off + n].view(lin.rows, lin.cols)
                off += n
                g, v = self.params[lin.prefix + "weight_g"], self.params[lin.prefix + "weight_v"]
                descs.append(_capi.WnDesc(g.data_ptr(), v.data_ptr(), lin.weff.data_ptr(), lin.gweff.data_ptr(),
                                          self.grad_view(lin.prefix + "weight_g").data_ptr(),
                                          self.grad_view(lin.prefix + "weight_v").data_ptr(), lin.rows, lin.cols))
            else:
                lin.weff = self.params[lin.prefix + "weight"]
                lin.gweff = self.grad_view(lin.prefix + "weight")
        self._n_desc = len(descs)
        self._max_rows = max(l.rows for l in self.linears.values())
        self._desc_dev = _lib.device_table(_capi.WnDesc, descs, dev) if descs else None

    def weights_changed(self):
        """Parameter memory was written behind PyTorch's back (the optimiser kernel): the derived operands are stale."""
        self._dirty = True

    def _prepare_weights(self, st):
        """Weight-norm products and packed Fourier blocks, rebuilt when a parameter was written."""
        try:
            sig = tuple(self.params[n]._version for n in self.param_names)
        except RuntimeError:      # inference tensors carry no version counter: rebuild every pass
            sig = None
        if not self._dirty and sig is not None and sig == self._derived_sig:
            return
        lib = _lib.get_lib()
        if self._desc_dev is not None:
            self._k("weightnorm_fwd", lib.ffno_weightnorm_fwd, _p(self._desc_dev), self._n_desc, self._max_rows, st)
        for names, packs in zip(self._fw_sets, self.packs):
            for w in range(self.nd):
                self._k("wide_pack_fw", lib.ffno_bgemm_pack_fw, _p(self.params[names[w]]), _p(packs[w]), self.C, self.Ks[w], st)
        self._derived_sig, self._dirty = sig, False

    def _table(self, L: int, K: int):
        t = self._tables.get((L, K))
        if t is None:
            F, Fi = dft_tables(L, K)
            t = self._tables[(L, K)] = (torch.from_numpy(F).to(self.device), torch.from_numpy(Fi).to(self.device))
        return t

    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def _gemm(ops, name, A, B, D, M, N, K, a, b, d, G0=1, G1=1, bias=None, gate=None, resid=None, relu=0, acc=0, split=False):
        """Record D = epilogue(A . B); a / b / d = (row, column[, batch 0, batch 1]) strides in floats."""
        ds = _capi.BgemmDesc()
        ds.A, ds.B, ds.D = A.data_ptr(), B.data_ptr(), D.data_ptr()
        ds.bias = None if bias is None else bias.data_ptr()
        ds.gate = None if gate is None else gate.data_ptr()
        ds.resid = None if resid is None else resid.data_ptr()
        for t, s in (("a", a), ("b", b), ("d", d)):
            s = tuple(s) + (0,) * (4 - len(s))
            for f, v in zip(("rs", "cs", "g0", "g1"), s):
                setattr(ds, f"{t}_{f}", int(v))
        ds.M, ds.N, ds.K, ds.G0, ds.G1 = int(M), int(N), int(K), int(G0), int(G1)
        ds.alpha, ds.relu, ds.accumulate = 1.0, int(relu), int(acc)
        ops.append(("gemm_split" if split else "gemm", name, ds, (A, B, D, bias, gate, resid)))

    @staticmethod
    def _ff(ops, name, S, W1, b1, W2, b2, resid, out, P, C, H) -> bool:
        """Record out = relu(S W1^T + b1) W2^T + b2 (+ resid) as one launch; False (nothing recorded) if the kernel refuses it."""
        ds = _capi.BgemmFfDesc()
        ds.S, ds.W1, ds.b1, ds.W2, ds.b2, ds.out = (t.data_ptr() for t in (S, W1, b1, W2, b2, out))
        ds.resid = None if resid is None else resid.data_ptr()
        ds.P, ds.s_rs, ds.out_rs, ds.resid_rs, ds.C, ds.H = int(P), C, C, C, C, H
        if not (W1.is_contiguous() and W2.is_contiguous()) or not _lib.get_lib().ffno_bgemm_ff_supported(ctypes.byref(ds)):
            return False
        ops.append(("ff", name, ds, (S, W1, b1, W2, b2, resid, out)))
        return True

    def _colsum(self, ops, ws, name, X, P, N, out):
        lib = _lib.get_lib()
        ops.append(("call", name, lib.ffno_bgemm_colsum, (_p(X), N, P, N, _p(ws.cpart), _p(out), 0), (X, out)))

    def _finish(self, ws, ops):
        """Recorded ops -> (name, function, arguments) with the shared split-K partial buffer sized for the largest user."""
        lib = _lib.get_lib()
        need = max([int(lib.ffno_bgemm_splitk_ws_floats(ctypes.byref(o[2]))) for o in ops if o[0] == "gemm_split"] + [1])
        if ws.part is None or ws.part.numel() < need:      # (the earlier, smaller buffer stays with the pass recorded over it)
            ws.part = torch.empty(need, dtype=torch.float32, device=self.device)
            ws.parts.append(ws.part)
        out = []
        for o in ops:
            if o[0] == "ff":
                out.append((o[1], lib.ffno_bgemm_ff, (ctypes.byref(o[2]),), o[2:]))
            elif o[0] == "gemm":
                if not lib.ffno_bgemm_supported(ctypes.byref(o[2])):
                    raise ValueError(f"{o[1]}: the GEMM kernels do not take this shape")
                out.append((o[1], lib.ffno_bgemm, (ctypes.byref(o[2]),), o[2:]))
            elif o[0] == "gemm_split":
                out.append((o[1], lib.ffno_bgemm_splitk, (ctypes.byref(o[2]), _p(ws.part)), o[2:]))
            else:
                out.append((o[1], o[2], o[3], o[4]))
        return out

    def _run(self, ops, st):
        for name, fn, args, _keep in ops:
            self._k(name, fn, *args, st)

    # ------------------------------------------------------------------------------------------------
    def _padded(self, sizes):
        return tuple(int(s) + self.pad for s in sizes)

    def _workspace(self, B, sizes, save):
        """``sizes``: the spatial extents of the DATA grid; the layers run on ``sizes + padding``."""
        fused = bool(self.fuse_ff) and not save
        key = (B, *sizes, bool(save), fused)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        S = self._padded(sizes)
        if any(K > S[d] // 2 for K, d in zip(self.Ks, self.axis_of_weight)):
            raise ValueError(f"modes={self.Ks} (in fourier_weight order: axes {self.axis_of_weight}) need 1 <= K <= L // 2 on the "
                             f"{' x '.join(map(str, S))} grid" + (f" ({' x '.join(map(str, sizes))} + {self.pad})" if self.pad else ""))
        C, H, L, Cin, O = self.C, self.H, self.L, self.Cin, self.O
        P, Pd = B * _prod(S), B * _prod(sizes)            # pixels of the padded grid (the layers) and of the data grid (lift, head)
        if P * max(H, 2 * C) >= 2 ** 38:
            raise ValueError("batch too large for one launch")
        f32 = dict(dtype=torch.float32, device=self.device)
        ws = type("WS", (), {})()
        ws.P, ws.Pd, ws.part, ws.parts, ws.shape, ws.saves, ws.fused = P, Pd, None, [], (B, *sizes), bool(save), fused
        nslot = L if save else 1
        lines = [P // S[d] for d in self.axis_of_weight]                     # per Fourier weight
        ws.x = torch.empty(Pd, Cin, **f32)
        ws.X = [torch.empty(P, C, **f32) for _ in range(2)]                  # layer inputs, ping-pong
        ws.S = [torch.empty(P, C, **f32) for _ in range(nslot)]              # spectral output = feed-forward input
        # hidden activations (their sign = the ReLU gate); none where the pass keeps h on the CU (the fused feed-forward launch)
        ws.Hh = [] if fused else [torch.empty(P, H, **f32) for _ in range(nslot)]
        # forward spectra [line][k][re / im][C], per Fourier weight and slot
        ws.SP = [[torch.empty(R, 2 * K * C, **f32) for _ in range(nslot)] for R, K in zip(lines, self.Ks)]
        ws.SM = torch.empty(max(R * 2 * K for R, K in zip(lines, self.Ks)) * C, **f32)      # mixed spectrum / adjoint spectrum
        ws.SD = torch.empty_like(ws.SM)
        ws.Bout = torch.empty(P, C, **f32)                                   # backcast of the last layer
        if self.pad:
            ws.sizes_c, ws.pads_c = (ctypes.c_int * self.nd)(*sizes), (ctypes.c_int * self.nd)(*[self.pad] * self.nd)      # host arrays
            if not _lib.get_lib().ffno_pad_supported(self.nd, ws.sizes_c, ws.pads_c, C):
                raise ValueError(f"the pad / crop kernels do not take a {sizes} grid padded by {self.pad}")
            ws.Dn = torch.empty(Pd, C, **f32)                                # dense: the lift's output; in the backward pass dL/d(it)
            ws.Bd = torch.empty(Pd, C, **f32)                                # the cropped last backcast (the head's input)
        else:
            ws.Dn, ws.Bd = None, ws.Bout
        ws.T0 = torch.empty(Pd, HEAD_DIM, **f32)
        ws.y = torch.empty(Pd, O, **f32)
        ws.cpart = torch.empty(int(_lib.get_lib().ffno_bgemm_colsum_ws_floats(P, max(H, HEAD_DIM, C))), **f32)
        ws.slot = (lambda l: l) if save else (lambda l: 0)
        ws.fwd = self._record_forward(ws, B, sizes)
        ws.bwd = ws.bwd_dx = None
        if save:
            ws.gy = torch.empty(Pd, O, **f32)
            ws.DT0 = torch.empty(Pd, HEAD_DIM, **f32)
            ws.G = [torch.empty(P, C, **f32) for _ in range(3)]
            ws.DH = torch.empty(P, H, **f32)
            ws.DS = torch.empty(P, C, **f32)
            ws.GW = torch.empty(max(self.Ks) * 4 * C * C, **f32)            # block gradient of one Fourier weight
            ws.dx = torch.empty(Pd, Cin, **f32)
            ws.bwd, ws.bwd_dx = self._record_backward(ws, B, sizes)
        self._ws[key] = ws
        while len(self._ws) > 4:
            self._ws.pop(next(iter(self._ws)))
        return ws

    def _axes(self, B, S):
        """Per spectral axis of the (padded) grid ``S``, the LAST axis first: (weight index, K, L, lines, G0, G1, (row, g0, g1)
        strides of a line's [L x C] image in a [P, C] tensor).  With inner = the product of the sizes after axis d, a line has row
        stride inner C; batch level 0 walks the inner positions (stride C), level 1 (b, the axes before d) (stride L inner C).  The
        lines of the last axis are contiguous and need one level."""
        C, out = self.C, []
        for d in range(self.nd - 1, -1, -1):
            w = self.axis_of_weight.index(d)
            Ln, inner, outer = S[d], _prod(S[d + 1:]), B * _prod(S[:d])
            if inner == 1:
                out.append((w, self.Ks[w], Ln, outer, outer, 1, (C, Ln * C, 0)))
            else:
                out.append((w, self.Ks[w], Ln, outer * inner, inner, outer, (inner * C, C, Ln * inner * C)))
        return out

    def _pad_op(self, ops, ws, name, crop, src, dst):
        """Record dense -> padded (embed) or padded -> dense (crop) of a [pixels, C] tensor (csrc/meshpad.hip)."""
        lib = _lib.get_lib()
        ops.append(("call", name, lib.ffno_pad_crop if crop else lib.ffno_pad_embed,
                    (_p(src), _p(dst), ws.shape[0], self.nd, ws.sizes_c, ws.pads_c, self.C), (src, dst)))

    def _record_forward(self, ws, B, sizes):
        C, H, L, Cin, O, P, Pd = self.C, self.H, self.L, self.Cin, self.O, ws.P, ws.Pd
        lin = self.linears
        bias = lambda pfx: self.params[pfx + "bias"]      # noqa: E731
        ops = []
        g = self._gemm
        axes = self._axes(B, self._padded(sizes))
        # the lift runs on the data grid (mesh_2d.py:149-150, mesh_3d.py:164-165); the embed rewrites ALL of the ping-pong buffer it
        # targets on every pass, zeros included
        lifted = ws.Dn if self.pad else ws.X[0]
        g(ops, "wide_lift", ws.x, lin["in_proj."].weff, lifted, Pd, C, Cin, (Cin, 1), (1, Cin), (C, 1), bias=bias("in_proj."))
        if self.pad:
            self._pad_op(ops, ws, "wide_pad_embed", False, ws.Dn, ws.X[0])
        for l in range(L):
            sl = ws.slot(l)
            X, Xn, S = ws.X[l % 2], ws.X[(l + 1) % 2], ws.S[sl]
            packs = self.packs[self._fw_set_of[l]]
            for i, (w, K, Ln, R, G0, G1, (rs, s0, s1)) in enumerate(axes):      # the layer's spectral output: the sum of the branches
                F, Fi = self._table(Ln, K)
                SP = ws.SP[w][sl]
                kc = 2 * K * C
                g(ops, f"wide_dft{w}", F, X, SP, 2 * K, C, Ln, (Ln, 1), (rs, 1, s0, s1), (C, 1, kc, G0 * kc), G0, G1)
                g(ops, f"wide_mix{w}", SP, packs[w], ws.SM, R, 2 * C, 2 * C, (kc, 1, 2 * C), (2 * C, 1, 4 * C * C), (kc, 1, 2 * C), K)
                g(ops, f"wide_idft{w}", Fi, ws.SM, S, Ln, C, 2 * K, (2 * K, 1), (C, 1, kc, G0 * kc), (rs, 1, s0, s1), G0, G1,
                  acc=int(i > 0))
            pfx = self.ff_prefix[l]
            l0, l1 = pfx + "layers.0.0.", pfx + "layers.1.0."
            # the head reads the last BACKCAST, not x + b (grid_2d.py:175)
            if ws.fused and self._ff(ops, "wide_ff", S, lin[l0].weff, bias(l0), lin[l1].weff, bias(l1), X if l < L - 1 else None,
                                     Xn if l < L - 1 else ws.Bout, P, C, H):
                continue
            if not ws.Hh:     # (the fused launch refused this layer: the pair, on one hidden image)
                ws.Hh = [torch.empty(P, H, dtype=torch.float32, device=self.device)]
            Hh = ws.Hh[sl]
            g(ops, "wide_ff1", S, lin[l0].weff, Hh, P, H, C, (C, 1), (1, C), (H, 1), bias=bias(l0), relu=1)
            if l < L - 1:
                g(ops, "wide_ff2", Hh, lin[l1].weff, Xn, P, C, H, (H, 1), (1, H), (C, 1), bias=bias(l1), resid=X)
            else:
                g(ops, "wide_ff2", Hh, lin[l1].weff, ws.Bout, P, C, H, (H, 1), (1, H), (C, 1), bias=bias(l1))
        if self.pad:      # the head runs on the data grid (mesh_2d.py:158-161, mesh_3d.py:173-176)
            self._pad_op(ops, ws, "wide_pad_crop", True, ws.Bout, ws.Bd)
        g(ops, "wide_head0", ws.Bd, lin["out.0."].weff, ws.T0, Pd, HEAD_DIM, C, (C, 1), (1, C), (HEAD_DIM, 1), bias=bias("out.0."))
        g(ops, "wide_head1", ws.T0, lin["out.1."].weff, ws.y, Pd, O, HEAD_DIM, (HEAD_DIM, 1), (1, HEAD_DIM), (O, 1), bias=bias("out.1."))
        return self._finish(ws, ops)

    def _record_backward(self, ws, B, sizes):
        lib = _lib.get_lib()
        C, H, L, Cin, O, P, Pd = self.C, self.H, self.L, self.Cin, self.O, ws.P, ws.Pd
        lin = self.linears
        gb = lambda pfx: self.grad_view(pfx + "bias")      # noqa: E731
        ops = []
        g, cs = self._gemm, self._colsum
        axes = self._axes(B, self._padded(sizes))
        o0, o1 = lin["out.0."], lin["out.1."]
        # head: y = T0 W1^T + b1,  T0 = Bd W0^T + b0, on the data grid; its input gradient is embedded into a zero padded one
        g(ops, "wide_head1_dw", ws.gy, ws.T0, o1.gweff, O, HEAD_DIM, Pd, (1, O), (HEAD_DIM, 1), (HEAD_DIM, 1), split=True)
        cs(ops, ws, "wide_head1_db", ws.gy, Pd, O, gb("out.1."))
        g(ops, "wide_head1_bwd", ws.gy, o1.weff, ws.DT0, Pd, HEAD_DIM, O, (O, 1), (HEAD_DIM, 1), (HEAD_DIM, 1))
        g(ops, "wide_head0_dw", ws.DT0, ws.Bd, o0.gweff, HEAD_DIM, C, Pd, (1, HEAD_DIM), (C, 1), (C, 1), split=True)
        cs(ops, ws, "wide_head0_db", ws.DT0, Pd, HEAD_DIM, gb("out.0."))
        g(ops, "wide_head0_bwd", ws.DT0, o0.weff, ws.Dn if self.pad else ws.G[0], Pd, C, HEAD_DIM, (HEAD_DIM, 1), (C, 1), (C, 1))
        if self.pad:
            self._pad_op(ops, ws, "wide_pad_embed", False, ws.Dn, ws.G[0])
        cur, gx = 0, None                # ws.G[cur]: dL/d(backcast of layer l);  gx: dL/dx_{l+1} (None above the last layer)
        seen = set()
        for l in range(L - 1, -1, -1):
            sl = ws.slot(l)
            S, Hh, Gb = ws.S[sl], ws.Hh[sl], ws.G[cur]
            pfx = self.ff_prefix[l]
            l0, l1 = pfx + "layers.0.0.", pfx + "layers.1.0."
            g(ops, "wide_ff2_dw", Gb, Hh, lin[l1].gweff, C, H, P, (1, C), (H, 1), (H, 1), split=True)
            cs(ops, ws, "wide_ff2_db", Gb, P, C, gb(l1))
            g(ops, "wide_ff2_bwd", Gb, lin[l1].weff, ws.DH, P, H, C, (C, 1), (H, 1), (H, 1), gate=Hh)
            g(ops, "wide_ff1_dw", ws.DH, S, lin[l0].gweff, H, C, P, (1, H), (C, 1), (C, 1), split=True)
            cs(ops, ws, "wide_ff1_db", ws.DH, P, H, gb(l0))
            g(ops, "wide_ff1_bwd", ws.DH, lin[l0].weff, ws.DS, P, C, H, (H, 1), (C, 1), (C, 1))
            # dL/dx_l = (dL/dx_{l+1}, the residual) + the adjoints of the two spectral branches
            nxt = [i for i in range(3) if i != cur and (gx is None or ws.G[i] is not gx)][0]
            Gn = ws.G[nxt]
            packs = self.packs[self._fw_set_of[l]]
            names = self.fw_names[l]
            for i, (w, K, Ln, R, G0, G1, (rs, s0, s1)) in enumerate(axes):
                F, Fi = self._table(Ln, K)
                SP = ws.SP[w][sl]
                kc = 2 * K * C
                g(ops, f"wide_idft{w}_adj", Fi, ws.DS, ws.SD, 2 * K, C, Ln, (1, 2 * K), (rs, 1, s0, s1), (C, 1, kc, G0 * kc), G0, G1)
                g(ops, f"wide_fw{w}_grad", SP, ws.SD, ws.GW, 2 * C, 2 * C, R, (1, kc, 2 * C), (kc, 1, 2 * C), (2 * C, 1, 4 * C * C), K,
                  split=True)
                ops.append(("call", f"wide_fw{w}_fold", lib.ffno_bgemm_fold_fw,
                            (_p(ws.GW), _p(self.grad_view(names[w])), C, K, int(names[w] in seen)), ()))
                seen.add(names[w])
                g(ops, f"wide_mix{w}_adj", ws.SD, packs[w], ws.SM, R, 2 * C, 2 * C, (kc, 1, 2 * C), (1, 2 * C, 4 * C * C), (kc, 1, 2 * C), K)
                g(ops, f"wide_dft{w}_adj", F, ws.SM, Gn, Ln, C, 2 * K, (1, Ln), (C, 1, kc, G0 * kc), (rs, 1, s0, s1), G0, G1,
                  resid=gx if i == 0 else None, acc=int(i > 0))
            gx, cur = Gn, nxt             # the block's residual x_{l+1} = x_l + b_l: both gradients are dL/dx_l from here on
        gl = ws.G[cur]
        if self.pad:                      # the adjoint of the embed after the lift
            self._pad_op(ops, ws, "wide_pad_crop", True, gl, ws.Dn)
            gl = ws.Dn
        g(ops, "wide_lift_dw", gl, ws.x, lin["in_proj."].gweff, C, Cin, Pd, (1, C), (Cin, 1), (Cin, 1), split=True)
        cs(ops, ws, "wide_lift_db", gl, Pd, C, gb("in_proj."))
        if self._desc_dev is not None:
            ops.append(("call", "weightnorm_bwd", lib.ffno_weightnorm_bwd, (_p(self._desc_dev), self._n_desc, self._max_rows), ()))
        dx_ops = []
        g(dx_ops, "wide_lift_bwd", gl, lin["in_proj."].weff, ws.dx, Pd, Cin, C, (C, 1), (Cin, 1), (Cin, 1))
        return self._finish(ws, ops), self._finish(ws, dx_ops)

    # ------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, save_for_backward: bool, training=None, own_output: bool = True) -> torch.Tensor:
        """x [B, *spatial, input_dim] -> [B, *spatial, output_dim]; ``own_output=False`` returns a view of the engine's buffer."""
        _lib.require_device_tensor(x, "x")
        if x.dim() != self.nd + 2 or x.shape[-1] != self.Cin:
            raise ValueError(f"expected x of shape [B, {'M, N' if self.nd == 2 else 'X, Y, Z'}, {self.Cin}], got {tuple(x.shape)}")
        if not self.params:
            raise RuntimeError("bind() the parameters first")
        B, *sizes = (int(v) for v in x.shape[:-1])
        ws = self._workspace(B, tuple(sizes), save_for_backward)
        st = _lib.current_stream(self.device)
        self._issue_stream = st
        self._prepare_weights(st)
        ws.x.copy_(x.reshape(ws.Pd, self.Cin))
        self._run(ws.fwd, st)
        self._saved = ws if save_for_backward else None
        self._last = ws
        y = ws.y.view(*ws.shape, self.O)
        return y.clone() if own_output else y

    def backward(self, gy: torch.Tensor, need_dx: bool = False) -> torch.Tensor:
        """gy = dL/doutput [B, *spatial, output_dim] -> the flat gradient buffer (``param_names`` order); ``self.dx`` with
        ``need_dx``."""
        _lib.require_device_tensor(gy, "gy")
        ws = self._saved
        if ws is None:
            raise RuntimeError("backward() needs a preceding forward(save_for_backward=True)")
        self._saved = None
        st = _lib.current_stream(self.device)
        self._issue_stream = st
        ws.gy.copy_(gy.reshape(ws.Pd, self.O))
        self._run(ws.bwd, st)
        self.dx = None
        if need_dx:
            self._run(ws.bwd_dx, st)
            self.dx = ws.dx.view(*ws.shape, self.Cin).clone()
        return self.gflat

    def relu_active_sets(self) -> Dict[Tuple[str, int], torch.Tensor]:
        """{("backcast", layer): [pixels of the padded grid, hidden] bool}: the ReLU decisions of the last
        forward(save_for_backward=True) (tests: the oracle is evaluated on the same linear piece)."""
        ws = getattr(self, "_last", None)
        if ws is None or not ws.saves:
            raise RuntimeError("relu_active_sets() needs a preceding forward(save_for_backward=True)")
        return {("backcast", l): ws.Hh[l] > 0 for l in range(self.L)}

    def workspace_bytes_per_layer(self, B: int, *sizes: int) -> int:
        """What one more layer keeps for the backward pass on a ``sizes`` data grid: s, h and the forward spectrum of every axis, at
        the pixel count of the padded grid."""
        S = self._padded(sizes)
        P = B * _prod(S)
        return 4 * (P * (self.C + self.H) + 2 * self.C * sum(P // S[d] * K for K, d in zip(self.Ks, self.axis_of_weight)))

    def forward_workspace_bytes(self, B: int, *sizes: int, fused=None) -> int:
        """The bytes of every tensor a forward-only pass (``forward(save_for_backward=False)``) keeps for a batch of ``B`` on a
        ``sizes`` data grid, without allocating them; ``fused``: with the fused feed-forward launch (default: ``fuse_ff``), which
        needs no [pixels, hidden] image -- exactly 4 P H bytes less, P the pixels of the padded grid."""
        fused = bool(self.fuse_ff) if fused is None else bool(fused)
        S = self._padded(sizes)
        C, H = self.C, self.H
        P, Pd = B * _prod(S), B * _prod(sizes)
        lines = [(P // S[d], K) for K, d in zip(self.Ks, self.axis_of_weight)]
        n = Pd * self.Cin + 4 * P * C + (0 if fused else P * H)                      # x; X (two), S, Bout; Hh
        n += sum(R * 2 * K * C for R, K in lines) + 2 * max(R * 2 * K for R, K in lines) * C      # SP; SM, SD
        n += (2 * Pd * C if self.pad else 0) + Pd * (HEAD_DIM + self.O)              # Dn, Bd; T0, y
        n += int(_lib.get_lib().ffno_bgemm_colsum_ws_floats(P, max(H, HEAD_DIM, C))) + 1      # cpart; part
        return 4 * n


class WideFFNO2DEngine(WideFFNOEngine):
    """FNOFactorized2DBlock: [B, M, N, input_dim] -> forecast [B, M, N, 1]; modes = one count, or (K_y, K_x) in fourier_weight order
    (fourier_weight[0] mixes the LAST axis, grid_2d.py:65-68, [1] the first, grid_2d.py:83-86)."""

    def __init__(self, *, modes, width: int, input_dim: int, n_layers: int, factor: int, share_weight: bool, **options):
        super().__init__(modes=modes, width=width, input_dim=input_dim, n_layers=n_layers, factor=factor, share_weight=share_weight,
                         axis_of_weight=(1, 0), padding=0, output_dim=1, **options)


class WideFFNOMeshEngine(WideFFNOEngine):
    """FNOFactorizedMesh2D / FNOFactorizedMesh3D with the keyword arguments the two modules hand FFNOEngine: [B, X, Y(, Z),
    input_dim] (coordinate channels included) -> [B, X, Y(, Z), output_dim].  fourier_weight[d] mixes axis d with modes[d]
    (mesh_2d.py:71-96, mesh_3d.py:62-103); the lift and the head run on the data grid, the layers on the grid padded by
    ``padding`` at the end of every axis (mesh_2d.py:150,158, mesh_3d.py:165,173)."""

    def __init__(self, *, modes, width: int, input_dim: int, n_layers: int, factor: int, share_weight: bool,
                 spatial_dims: int = 2, padding: int = 0, output_dim: int = 1, first_axis_first: bool = True, **options):
        if spatial_dims not in (2, 3):
            raise ValueError("spatial_dims must be 2 or 3")
        if spatial_dims == 2 and not first_axis_first:
            raise ValueError("fourier_weight[0] on the last axis is the grid block's order: WideFFNO2DEngine")
        if not isinstance(modes, (tuple, list)) or len(modes) != spatial_dims:
            raise ValueError("one mode count per spatial axis")
        super().__init__(modes=modes, width=width, input_dim=input_dim, n_layers=n_layers, factor=factor, share_weight=share_weight,
                         axis_of_weight=tuple(range(spatial_dims)), padding=padding, output_dim=output_dim, **options)
