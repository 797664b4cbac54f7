"""Fused feed-forward of the wide block (fourierflow_amd/csrc/bgemm_ff.hip: ffno_bgemm_ff) through the C ABI, against the pair of
ffno_bgemm launches it replaces (bit for bit: same instruction, same summation order) and against fp64 numpy (the bar
test_kernels_bgemm.py sets for v_mfma_f32_32x32x2_f32).  Shapes are the smallest at which the tiling can go wrong: one row, just
over a 32-row MFMA tile, just over the 128-row workgroup tile, a tile turn-over; H = C, an odd multiple of 32, the largest
supported shape, a single H chunk.  CPU wave emulator (-m "not gpu") and MI355X (-m gpu)."""
import ctypes

import numpy as np
import pytest

from backend_util import be, rel_l2  # noqa: F401
from test_kernels_bgemm import f64, make_desc, rnd

TOL = 1e-5
GUARD = 4      # rows behind row P - 1 of `out` that no launch may touch


def ff_desc(be, S, W1, b1, W2, b2, resid, out, P, C, H, ld):
    from fourierflow_amd._capi import BgemmFfDesc
    ds = BgemmFfDesc()
    for name, h in (("S", S), ("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2), ("resid", resid), ("out", out)):
        setattr(ds, name, None if h is None else be.ptr(h).value)
    ds.P, ds.s_rs, ds.out_rs, ds.resid_rs, ds.C, ds.H = P, ld, ld, ld, C, H
    ds.keep = (S, W1, b1, W2, b2, resid, out)      # the descriptor holds raw addresses
    return ds


class Case:
    """Operands of one (P, C, H) on the backend, rows C + 8 floats apart, and what the fused launch / the pair give."""

    def __init__(self, be, P, C, H, seed, b1=None):
        rs = np.random.RandomState(seed)
        self.be, self.P, self.C, self.H, self.ld = be, P, C, H, C + 8
        self.S, self.R = rnd(rs, P, self.ld), rnd(rs, P, self.ld)
        self.W1, self.W2 = rnd(rs, H, C) / np.float32(np.sqrt(C)), rnd(rs, C, H) / np.float32(np.sqrt(H))
        self.b1 = rnd(rs, H) if b1 is None else np.full(H, b1, np.float32)      # random: about half the units are dead
        self.b2 = rnd(rs, C)
        self.d = {n: be.put(getattr(self, n)) for n in ("S", "R", "W1", "W2", "b1", "b2")}

    def fused(self, resid):
        be, d = self.be, self.d
        out = be.empty((self.P + GUARD, self.ld))
        ds = ff_desc(be, d["S"], d["W1"], d["b1"], d["W2"], d["b2"], d["R"] if resid else None, out, self.P, self.C, self.H, self.ld)
        assert be.lib.ffno_bgemm_ff_supported(ctypes.byref(ds)) == 1
        assert be.lib.ffno_bgemm_ff(ctypes.byref(ds), None) == 0
        return np.array(be.get(out), copy=True)

    def pair(self, resid, relu=1):
        be, d, P, C, H, ld = self.be, self.d, self.P, self.C, self.H, self.ld
        h, out = be.empty((P, H)), be.empty((P + GUARD, ld))
        d1 = make_desc(be, d["S"], d["W1"], h, P, H, C, (ld, 1), (1, C), (H, 1), bias=d["b1"], relu=relu)
        d2 = make_desc(be, h, d["W2"], out, P, C, H, (H, 1), (1, H), (ld, 1), bias=d["b2"], resid=d["R"] if resid else None)
        assert be.lib.ffno_bgemm(ctypes.byref(d1), None) == 0
        assert be.lib.ffno_bgemm(ctypes.byref(d2), None) == 0
        return np.array(be.get(out), copy=True)

    def ref64(self, resid):
        C = self.C
        h = np.maximum(f64(self.S[:, :C]) @ f64(self.W1).T + f64(self.b1), 0)
        return h @ f64(self.W2).T + f64(self.b2) + (f64(self.R[:, :C]) if resid else 0.0)

    def check(self):
        P, C = self.P, self.C
        for resid in (True, False):
            got = self.fused(resid)
            assert np.isnan(got[P:]).all() and np.isnan(got[:P, C:]).all(), "guard rows / row padding written"
            assert not np.isnan(got[:P, :C]).any()
            assert np.array_equal(got[:P, :C], self.pair(resid)[:P, :C]), ("not the pair's bits", P, C, self.H, resid)
            assert rel_l2(got[:P, :C], self.ref64(resid)) < TOL, (P, C, self.H, resid)


@pytest.mark.parametrize("P", [1, 33, 130, 257])
def test_bgemm_ff_row_tile_edges(be, P):
    Case(be, P, 96, 384, seed=P).check()


@pytest.mark.parametrize("C,H", [(96, 96), (160, 640), (256, 1024), (224, 32)])
def test_bgemm_ff_channel_and_chunk_edges(be, C, H):
    Case(be, 33, C, H, seed=C + H).check()


def test_bgemm_ff_all_units_dead(be):
    """b1 = -1e3 on every unit: h = 0, the result is b2 + resid exactly."""
    c = Case(be, 33, 96, 384, seed=1, b1=-1e3)
    got = c.fused(True)[:33, :96]
    assert np.array_equal(got, c.b2[None, :] + c.R[:, :96])
    assert np.array_equal(c.fused(False)[:33, :96], np.broadcast_to(c.b2, (33, 96)))


def test_bgemm_ff_relu_never_clips(be):
    """b1 = +1e3: the result is the two plain products (the pair without its ReLU)."""
    c = Case(be, 33, 96, 384, seed=2, b1=1e3)
    for resid in (True, False):
        got = c.fused(resid)[:33, :96]
        assert np.array_equal(got, c.pair(resid, relu=0)[:33, :96])
        assert rel_l2(got, c.ref64(resid)) < TOL


def test_bgemm_ff_two_runs_bit_identical(be):
    c = Case(be, 130, 128, 512, seed=3)
    assert np.array_equal(c.fused(True), c.fused(True), equal_nan=True)


def test_bgemm_ff_argument_checks(be):
    lib = be.lib
    P = 8

    def operands(C, H, ld):
        z = be.zeros
        return dict(S=z((P, ld)), W1=z((H, C)), b1=z(H), W2=z((C, H)), b2=z(C), resid=z((P, ld)), out=z((P, ld)))

    def refused(ds):
        return lib.ffno_bgemm_ff_supported(ctypes.byref(ds)) == 0 and lib.ffno_bgemm_ff(ctypes.byref(ds), None) < 0

    o = operands(96, 384, 104)
    ok = ff_desc(be, P=P, C=96, H=384, ld=104, **o)
    assert lib.ffno_bgemm_ff_supported(ctypes.byref(ok)) == 1 and lib.ffno_bgemm_ff(ctypes.byref(ok), None) == 0
    nores = ff_desc(be, P=P, C=96, H=384, ld=104, **dict(o, resid=None))      # NULL resid is a shape, not an error
    assert lib.ffno_bgemm_ff_supported(ctypes.byref(nores)) == 1 and lib.ffno_bgemm_ff(ctypes.byref(nores), None) == 0
    assert lib.ffno_bgemm_ff_supported(None) == 0 and lib.ffno_bgemm_ff(None, None) == -1
    for C, H in ((64, 256), (80, 320), (288, 288), (96, 48), (96, 1056)):
        assert refused(ff_desc(be, P=P, C=C, H=H, ld=C + 8, **operands(C, H, C + 8))), (C, H)
    for field in ("s_rs", "out_rs", "resid_rs"):
        bad = ff_desc(be, P=P, C=96, H=384, ld=104, **o)
        setattr(bad, field, 92)                            # a row stride below C
        assert refused(bad), field
        setattr(bad, field, 102)                           # not a multiple of 4
        assert refused(bad), field
    for field in ("S", "W1", "W2", "resid", "out"):        # a misaligned base pointer
        bad = ff_desc(be, P=P, C=96, H=384, ld=104, **o)
        setattr(bad, field, getattr(bad, field) + 4)
        assert refused(bad), field
    bad = ff_desc(be, P=P, C=96, H=384, ld=104, **dict(o, out=o["S"]))
    assert refused(bad)
    bad = ff_desc(be, P=P, C=96, H=384, ld=104, **dict(o, out=o["resid"]))
    assert refused(bad)
    for field in ("S", "W1", "b1", "W2", "b2", "out"):
        bad = ff_desc(be, P=P, C=96, H=384, ld=104, **o)
        setattr(bad, field, None)
        assert lib.ffno_bgemm_ff(ctypes.byref(bad), None) == -1 and lib.ffno_bgemm_ff_supported(ctypes.byref(bad)) == 0, field
    bad = ff_desc(be, P=0, C=96, H=384, ld=104, **o)
    assert lib.ffno_bgemm_ff(ctypes.byref(bad), None) == -1
