"""The pointwise stage of a geo-FNO layer on its latent grid (csrc/plin.hip: ffno_plin_pos_fwd, ffno_plin_pos_bwd_weights;
reference zongyi_fno/point_cloud_2d.py:221-232) against numpy float64 models of
    pre = b + W x + add + gw[:, 0] gx(p) + gw[:, 1] gy(p),   out = act(pre)
and of its parameter gradients, within the TOL of tests/test_kernels_plin.py (2e-6 rel-L2: fp32 dot products in another
summation order).  Shapes (B, s1, s2, C): (2, 7, 9, 32) -- 126 points, a ragged second 64-point tile, two samples (a missing
modulo) and unequal axes (a swap); (3, 5, 13, 64); (1, 2, 2, 32), the two-point linspace."""
import numpy as np
import pytest

from backend_util import be, rel_l2  # noqa: F401
from test_kernels_plin import TOL, _dgelu, _gelu

SHAPES = [(2, 7, 9, 32), (3, 5, 13, 64), (1, 2, 2, 32)]


def _tables(s1, s2):
    return np.linspace(0, 1, s1).astype(np.float32), np.linspace(0, 1, s2).astype(np.float32)


def _coords(B, s1, s2):
    """gx(p), gy(p) of every point p = (sample, ix, iy), float64 values of the fp32 tables."""
    tx, ty = _tables(s1, s2)
    gx = np.broadcast_to(tx[None, :, None], (B, s1, s2)).reshape(-1).astype(np.float64)
    gy = np.broadcast_to(ty[None, None, :], (B, s1, s2)).reshape(-1).astype(np.float64)
    return gx, gy


def _data(B, s1, s2, C, seed=0, ld=None):
    rs = np.random.RandomState(seed)
    P, ld = B * s1 * s2, ld or C
    x = np.zeros((P, ld), np.float32)
    x[:, :C] = rs.standard_normal((P, C))
    W = (rs.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    b = rs.standard_normal(C).astype(np.float32)
    add = np.zeros((P, ld), np.float32)
    add[:, :C] = rs.standard_normal((P, C))
    gw = rs.standard_normal((C, 2)).astype(np.float32)
    return x, W, b, add, gw


def _fwd(be, x, W, b, add, gw, B, s1, s2, Cin, Cout, act_mode, ldx, ldo, want_pre=True):
    tx, ty = _tables(s1, s2)
    P = B * s1 * s2
    out, pre = be.empty((P, ldo)), (be.empty((P, ldo)) if want_pre else None)
    h = [be.put(a) for a in (x, W, b, add, gw, tx, ty)]
    rc = be.lib.ffno_plin_pos_fwd(be.ptr(h[0]), ldx, be.ptr(h[1]), be.ptr(h[2]), be.ptr(h[3]), be.ptr(h[4]), be.ptr(h[5]),
                                  be.ptr(h[6]), be.ptr(out), ldo, be.ptr(pre), B, s1, s2, Cin, Cout, act_mode, None)
    assert rc == 0
    return be.get(out), (be.get(pre) if want_pre else None)


@pytest.mark.parametrize("B,s1,s2,C", SHAPES)
@pytest.mark.parametrize("act_mode,with_add", [(0, True), (2, True), (2, False), (0, False)])
def test_plin_pos_forward(be, B, s1, s2, C, act_mode, with_add):
    x, W, b, add, gw = _data(B, s1, s2, C)
    got, pre = _fwd(be, x, W, b, add if with_add else None, gw, B, s1, s2, C, C, act_mode, C, C)
    gx, gy = _coords(B, s1, s2)
    ref_pre = x.astype(np.float64) @ W.astype(np.float64).T + b + np.outer(gx, gw[:, 0]) + np.outer(gy, gw[:, 1])
    if with_add:
        ref_pre = ref_pre + add
    ref = _gelu(ref_pre) if act_mode == 2 else ref_pre
    e, ep = rel_l2(got, ref), rel_l2(pre, ref_pre)
    print(f"[{B}x{s1}x{s2}x{C} act {act_mode} add {with_add}] out {e:.2e} pre {ep:.2e}")
    assert e < TOL and ep < TOL


@pytest.mark.parametrize("vec", [True, False])
def test_plin_pos_pad_channels_are_exact_zeros(be, vec):
    """20 live channels in a 32-wide (vector stores) or 30-wide (scalar stores) row."""
    B, s1, s2, C, ld = 2, 7, 9, 20, 32 if vec else 30
    x, W, b, add, gw = _data(B, s1, s2, C, seed=4, ld=ld)
    got, pre = _fwd(be, x, W, b, add, gw, B, s1, s2, C, C, 2, ld, ld)
    gx, gy = _coords(B, s1, s2)
    ref_pre = x[:, :C].astype(np.float64) @ W.astype(np.float64).T + b + add[:, :C] + np.outer(gx, gw[:, 0]) + np.outer(gy, gw[:, 1])
    assert rel_l2(got[:, :C], _gelu(ref_pre)) < TOL and rel_l2(pre[:, :C], ref_pre) < TOL
    assert not got[:, C:].any() and not pre[:, C:].any()


@pytest.mark.parametrize("B,s1,s2,C", SHAPES)
def test_plin_pos_position_term_alone(be, B, s1, s2, C):
    """W = 0, b = 0, no add: pre is gw . (gx, gy) alone."""
    x, W, b, _, gw = _data(B, s1, s2, C, seed=5)
    got, _ = _fwd(be, x, np.zeros_like(W), np.zeros_like(b), None, gw, B, s1, s2, C, C, 0, C, C, want_pre=False)
    gx, gy = _coords(B, s1, s2)
    ref = np.outer(gx, gw[:, 0]) + np.outer(gy, gw[:, 1])
    assert rel_l2(got, ref) < TOL
    # ... and the same without a linear term at all (x = W = NULL: the layer-0 stage)
    got0, _ = _fwd(be, None, None, np.zeros_like(b), None, gw, B, s1, s2, C, C, 0, C, C, want_pre=False)
    np.testing.assert_array_equal(got0, got)


@pytest.mark.parametrize("B,s1,s2,C", SHAPES)
@pytest.mark.parametrize("act_mode", [0, 2])
def test_plin_pos_is_plin_bit_for_bit_without_a_position_weight(be, B, s1, s2, C, act_mode):
    x, W, b, add, gw = _data(B, s1, s2, C, seed=6)
    got, pre = _fwd(be, x, W, b, add, np.zeros_like(gw), B, s1, s2, C, C, act_mode, C, C)
    P = B * s1 * s2
    out, pre0 = be.empty((P, C)), be.empty((P, C))
    h = [be.put(a) for a in (x, W, b, add)]
    assert be.lib.ffno_plin_fwd(be.ptr(h[0]), C, be.ptr(h[1]), be.ptr(h[2]), be.ptr(h[3]), be.ptr(out), C, None, None,
                                be.ptr(pre0), P, C, C, act_mode, None) == 0
    np.testing.assert_array_equal(got.view(np.int32), be.get(out).view(np.int32))
    np.testing.assert_array_equal(pre.view(np.int32), be.get(pre0).view(np.int32))


def test_plin_pos_keeps_a_negative_zero_without_a_position_weight(be):
    """-0 weights on positive inputs and a -0 bias give pre = -0 in ffno_plin_fwd; adding a zero position term must not turn
    it into +0."""
    B, s1, s2, C = 1, 2, 2, 32
    x = np.abs(_data(B, s1, s2, C, seed=9)[0]) + 1
    W, b = np.full((C, C), -0.0, np.float32), np.full(C, -0.0, np.float32)
    got, pre = _fwd(be, x, W, b, None, np.zeros((C, 2), np.float32), B, s1, s2, C, C, 0, C, C)
    assert np.signbit(got).all() and np.signbit(pre).all() and not got.any()


@pytest.mark.parametrize("B,s1,s2,C", SHAPES)
@pytest.mark.parametrize("act_mode,linear", [(2, True), (0, True), (2, False)])
def test_plin_pos_weight_gradients(be, B, s1, s2, C, act_mode, linear):
    x, _, _, _, _ = _data(B, s1, s2, C, seed=7)
    rs = np.random.RandomState(8)
    P = B * s1 * s2
    g = rs.standard_normal((P, C)).astype(np.float32)
    act = (rs.standard_normal((P, C)) * 1.5).astype(np.float32)         # the kept pre-activation
    dpre = g.astype(np.float64) * (_dgelu(act.astype(np.float64)) if act_mode == 2 else 1.0)
    gx, gy = _coords(B, s1, s2)
    tx, ty = _tables(s1, s2)
    hg, hact, hx, htx, hty = be.put(g), be.put(act), be.put(x) if linear else None, be.put(tx), be.put(ty)
    part = be.empty(int(be.lib.ffno_plin_wgrad_nsplit(P)) * C * (C + 3))
    dW0, db0, dgw0 = (rs.standard_normal(s).astype(np.float32) for s in ((C, C), (C,), (C, 2)))
    runs = []
    for accumulate in (0, 1, 0):
        dW, db, dgw, dp = be.put(dW0) if linear else None, be.put(db0), be.put(dgw0), be.empty((P, C))
        rc = be.lib.ffno_plin_pos_bwd_weights(be.ptr(hg), C, be.ptr(hact) if act_mode else None, be.ptr(hx), C, be.ptr(htx),
                                              be.ptr(hty), be.ptr(part), be.ptr(dW), be.ptr(db), be.ptr(dgw), be.ptr(dp), B, s1, s2,
                                              C, C, accumulate, act_mode, None)
        assert rc == 0
        got = [np.array(be.get(h)) for h in ((dW, db, dgw, dp) if linear else (db, dgw, dp))]
        runs.append(got)
        ref = [dpre.sum(0) + (db0 if accumulate else 0),
               np.stack([dpre.T @ gx, dpre.T @ gy], axis=1) + (dgw0 if accumulate else 0), dpre]
        if linear:
            ref.insert(0, dpre.T @ x.astype(np.float64) + (dW0 if accumulate else 0))
        for name, a, r in zip(("dW", "db", "dgw", "dpre") if linear else ("db", "dgw", "dpre"), got, ref):
            e = rel_l2(a, r)
            print(f"[{B}x{s1}x{s2}x{C} act {act_mode} linear {linear} acc {accumulate}] {name} {e:.2e}")
            assert e < TOL, name
    for a, c in zip(runs[0], runs[2]):          # no atomics: two runs give the same bits
        np.testing.assert_array_equal(a.view(np.int32), c.view(np.int32))


def test_plin_pos_rejects_bad_arguments(be):
    """Every refusal returns a status before anything is launched: the outputs keep their NaN fill."""
    B, s1, s2, C = 1, 2, 2, 8
    x, t = be.zeros((4, 8)), be.zeros(2)
    out = be.empty((4, 8))
    p = be.ptr
    f = be.lib.ffno_plin_pos_fwd
    assert f(p(x), 8, p(x), None, None, None, p(t), p(t), p(out), 8, None, B, s1, s2, C, C, 0, None) == -1       # gw
    assert f(p(x), 8, p(x), None, None, p(x), None, p(t), p(out), 8, None, B, s1, s2, C, C, 0, None) == -1       # tx
    assert f(p(x), 8, None, None, None, p(x), p(t), p(t), p(out), 8, None, B, s1, s2, C, C, 0, None) == -1       # x without W
    assert f(p(x), 4, p(x), None, None, p(x), p(t), p(t), p(out), 8, None, B, s1, s2, C, C, 0, None) == -1       # ldx < Cin
    assert f(p(x), 8, p(x), None, None, p(x), p(t), p(t), p(out), 4, None, B, s1, s2, C, C, 0, None) == -1       # ldo < Cout
    assert f(p(x), 8, p(x), None, None, p(x), p(t), p(t), p(out), 8, None, B, 0, s2, C, C, 0, None) == -1        # empty grid
    assert f(p(x), 8, p(x), None, None, p(x), p(t), p(t), p(out), 8, None, B, s1, s2, C, C, 3, None) == -1       # act_mode
    assert f(p(x), 200, p(x), None, None, p(x), p(t), p(t), p(out), 8, None, B, s1, s2, 200, C, 0, None) == -2   # Cin > 128
    assert np.isnan(be.get(out)).all()
    w = be.lib.ffno_plin_pos_bwd_weights
    dW, db, dgw, part = be.empty((8, 8)), be.empty(8), be.empty((8, 2)), be.empty(8 * 11)
    args = (B, s1, s2, C, C, 0, 0, None)
    assert w(None, 8, None, p(x), 8, p(t), p(t), p(part), p(dW), p(db), p(dgw), None, *args) == -1               # g
    assert w(p(x), 8, None, p(x), 8, p(t), p(t), p(part), p(dW), p(db), None, None, *args) == -1                 # dgw
    assert w(p(x), 8, None, p(x), 8, p(t), p(t), p(part), None, p(db), p(dgw), None, *args) == -1                # x without dW
    assert w(p(x), 8, None, p(x), 8, p(t), None, p(part), p(dW), p(db), p(dgw), None, *args) == -1               # ty
    assert w(p(x), 128, None, p(x), 128, p(t), p(t), p(part), p(dW), p(db), p(dgw), None, B, s1, s2, 128, 128, 0, 0, None) == -2
    for h in (dW, db, dgw, part):
        assert np.isnan(be.get(h)).all()
