"""The separable rfftn -> corner modes -> irfftn chain of the non-factorized operators (FNOPlus2DBlock, FNOZongyi2DBlock,
FNOMesh2D / FNOMesh3D, ops.modes_to_grid / ops.grid_to_mixed_modes), defined once; DESIGN.md section 4 "The corner chain".

Over a padded channels-last grid [B, *Sp, C] with Ks[a] retained modes on axis a:

    analysis :  ffno_dft_fwd along the last axis (Ks[-1] bins), then one complex row transform per remaining axis from the
                second-to-last to the first (ffno_cdft_rows_mfma, inverse = 0), each keeping the 2 Ks[a] corner rows
                (k' < Ks[a]: k = k', else k = k' - 2 Ks[a]) and treating the modes kept so far as columns
    mix      :  ffno_mode_mix over the retained modes with the B samples as rows
    synthesis:  the row transforms back in the opposite order (inverse = 1), then ffno_dft_inv (zero-padded spectrum)

The retained spectrum is mode-major, Z[k_last][k'_(n-2)]...[k'_0][b][re/im][c]; the twiddle tables carry 1 / sqrt(L)
(norm="ortho").  ``fwd=False`` swaps the c_k / conjugate flags: the adjoint of each part, on the same launches.
A chain allocates nothing: callers ask it how large buffers are, and it launches through their ``launch(name, fn, *args)``.
The engines pass ``lambda *a: self._k(*a)``, not the bound method, so that a ``_k`` replaced on the instance later (as the
tests do to record launches) still sees the chain's launches.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Sequence

from . import _capi, _lib

_p = _lib.ptr


def checked(name, fn, *args):
    """The plain launch wrapper: call and raise on a non-zero status."""
    _capi.check(fn(*args), name)


class RowPass(NamedTuple):
    """One ffno_cdft_rows_mfma launch: ``rows`` x ``cols`` lines of ``length`` points -> 2 ``kept`` corner rows each."""
    label: str
    rows: int
    length: int
    kept: int
    cols: int


class CornerChain:
    """Geometry and launches for B samples on the padded grid Sp, Ks modes per axis, C channels.  Bv, Mv, Nv, L, K, R, spec and
    modes read like the same attributes of an engine ``_View``: FFNOEngine lists the chain as the one view of spectral="plus"."""

    def __init__(self, B: int, Sp: Sequence[int], Ks: Sequence[int], C: int, launch, device):
        self.B, self.Sp, self.Ks, self.C = B, tuple(Sp), tuple(Ks), C
        self._launch, self.device = launch, device
        nd = len(Sp)
        # the last-axis line view [Bv, Mv, Nv, C] of the grid; L points and K bins per line
        self.Bv, self.Mv, self.Nv = B * math.prod(Sp[:-2]), Sp[-2], Sp[-1]
        self.L, self.K = Sp[-1], Ks[-1]
        sizes = [self.K * self.Bv * self.Mv * 2 * C]          # after dft_fwd: [k_last][line][2][C]
        self.passes: List[RowPass] = []
        cols = self.K
        for a in range(nd - 2, -1, -1):
            rows = B * math.prod(Sp[:a])
            label = "cdft_rows" if nd == 2 else "cdft_rows(%s)" % "xy"[a]
            self.passes.append(RowPass(label, rows, Sp[a], Ks[a], cols))
            cols *= 2 * Ks[a]
            sizes.append(cols * rows * 2 * C)                 # [modes so far][rows][2][C]
        self.modes = cols                        # retained modes: what the mix and the weight gradient run over
        self.R = B                               # ... with the samples as rows
        self.spec = sizes[-1]                    # floats of the retained spectrum [modes][B][2][C]
        self.mid_sizes = sizes[:-1]              # floats of the spectra between the stages, in analysis order
        self.planes_floats = 2 * cols * C * C    # floats of one [modes][2][C][C] set: packed weights, or one slice of fw_grad_partial
        lib = _lib.get_lib()
        self.cw_floats = max(int(lib.ffno_cdft_rows_ws_floats(p.rows, C, p.kept, p.cols)) for p in self.passes)
        # the tables of every transform length, from the package's one cache (which keeps them alive)
        self._tw = {L: _p(_lib.twiddle(L, device)) for L in Sp}

    def scratch(self, alloc):
        """What conv() needs besides its spectra, from the caller's ``alloc(floats)``: the spectra between the stages of the
        analysis and of the synthesis (mid_sizes each) and the row-transform scratch."""
        return [alloc(n) for n in self.mid_sizes], [alloc(n) for n in self.mid_sizes], alloc(self.cw_floats)

    # ---- launches ----------------------------------------------------------------------------------------------------
    def analysis(self, src, mid, z, cw, fwd: bool, st):
        """z = kept corners of rfftn(src) (``fwd``), or the adjoint of the zero-padded irfftn."""
        lib, C = _lib.get_lib(), self.C
        self._launch("dft_fwd", lib.ffno_dft_fwd, _p(src), _p(mid[0]), self._tw[self.L], self.Bv, self.Mv, self.Nv, C, self.K, 0,
                     0 if fwd else 1, st)
        bufs = list(mid) + [z]
        for i, p in enumerate(self.passes):
            self._launch(p.label, lib.ffno_cdft_rows_mfma, _p(bufs[i]), _p(bufs[i + 1]), _p(cw), self._tw[p.length], p.rows,
                         p.length, C, p.kept, p.cols, 0, st)

    def synthesis(self, z, mid, dst, cw, fwd: bool, st, resid=None, accumulate: int = 0):
        """dst (+)= [resid +] irfftn of the zero-padded corners z (``fwd``), or the adjoint of the corner rfftn."""
        lib, C = _lib.get_lib(), self.C
        bufs = list(mid) + [z]
        for i in range(len(self.passes) - 1, -1, -1):
            p = self.passes[i]
            self._launch(p.label, lib.ffno_cdft_rows_mfma, _p(bufs[i + 1]), _p(bufs[i]), _p(cw), self._tw[p.length], p.rows,
                         p.length, C, p.kept, p.cols, 1, st)
        self._launch("dft_inv", lib.ffno_dft_inv, _p(mid[0]), _p(dst), _p(resid), self._tw[self.L], self.Bv, self.Mv, self.Nv, C,
                     self.K, 0, 1 if fwd else 0, accumulate, st)

    def mix(self, z, planes, y, fwd: bool, st):
        """y[mode] = z[mode] x planes[mode] ([2][C][C] per retained mode; the adjoint takes the transposed set, conjugated)."""
        self._launch("mode_mix", _lib.get_lib().ffno_mode_mix, _p(z), _p(planes), _p(y), self.B, self.C, self.modes,
                     0 if fwd else 1, st)

    def conv(self, src, dst, z, y, planes, scr, fwd: bool, st, resid=None, accumulate: int = 0):
        """dst (+)= [resid +] irfftn(corner-mix(rfftn(src))), or its adjoint; z keeps the analysed spectrum, y the mixed one;
        scr = scratch()."""
        mid_a, mid_s, cw = scr
        self.analysis(src, mid_a, z, cw, fwd, st)
        self.mix(z, planes, y, fwd, st)
        self.synthesis(y, mid_s, dst, cw, fwd, st, resid, accumulate)

    def fw_grad_partial(self, sx, sd, part, st, nsplit: int = 1, n_layers: int = 1):
        """Per-mode partial weight gradients of ``n_layers`` consecutive saved spectra sx against the adjoint spectra sd."""
        self._launch("fw_grad_partial", _lib.get_lib().ffno_fw_grad_partial, _p(sx), _p(sd), _p(part), self.R, self.C, self.modes,
                     nsplit, 0, n_layers, self.spec, self.spec, st)
