"""ffno_prediction_export_step (include/ffno.h, csrc/ffno_pred_export.h; reference routines/grid_2d_markov.py:427-476 with
utils/array.py:50-80) through the C ABI, on the emulator and on the GPU, against the float64 restatement of tests/coarsen_oracle.py
(pinned by a closed form in tests/test_kernels_coarsen.py).  Inputs are that file's non-periodic fields.

Bounds (absolute, u = 2^-24, first order), as derived in tests/test_kernels_coarsen.py for the same arithmetic: the mean of a block
is a sequential fp32 sum of f terms in index order, (f - 1) u sum|x| <= (f - 1) f u max|x|, and one division by f, u |mean|:
|d u_c| <= f u max|u|, |d v_c| <= f u max|v|.  The curl inherits 2 f u max|v| / dx + 2 f u max|u| / dy and adds its own roundings;
that file's  c f u (max|v| / dx + max|u| / dy)  with c = 8 is taken over unchanged.  f = 1 is a copy: exact.
"""
import numpy as np
import pytest

import coarsen_oracle as co
from backend_util import be  # noqa: F401
from test_kernels_coarsen import _case

U = 2.0 ** -24
TWO_PI = 2 * np.pi
B, NS, T = 2, 3, 1
SENTINEL = np.float32(-12345.5)


def _run(be, vel, m, t=T, n_steps=NS, lx=TWO_PI, ly=TWO_PI):
    lib, p = be.lib, be.ptr
    Bv, X, Y, _ = vel.shape
    outs = [be.put(np.full((n_steps, Bv, m, m), SENTINEL, np.float32)) for _ in range(3)]
    rc = lib.ffno_prediction_export_step(p(be.put(vel)), p(outs[0]), p(outs[1]), p(outs[2]), Bv, X, Y, m, n_steps, t, lx, ly, None)
    assert rc == 0
    return [be.get(o).copy() for o in outs]


def _slices(m):
    """Slices of coarse rows per sample (include/ffno.h, ffno_vorticity_coarsen_step): about 1024 cells each."""
    rows = -(-m // min(m, -(-m * m // 1024)))
    return -(-m // rows)


def _untouched(outs, t):
    for o in outs:
        for k in range(o.shape[0]):
            if k != t:
                assert (o[k] == SENTINEL).all()


def test_export_at_the_models_own_size_copies_the_three_channels(be):
    vel, _ = _case(11, B, 8, 8, NS)
    outs = _run(be, vel, 8)
    for ch, o in enumerate(outs):      # vorticity, vx, vy = channels 0, 1, 2: the same bits
        assert o[T].tobytes() == np.ascontiguousarray(vel[..., ch]).tobytes()
    _untouched(outs, T)


@pytest.mark.parametrize("X,m,slices", [(16, 8, 1), (24, 8, 1), (80, 40, 2)])
def test_export_reduces_like_the_float64_oracle(be, X, m, slices):
    """(24, 8): f = 3, no power of two.  (80, 40): 1600 coarse cells, two slices of 20 rows per sample -- the halo row of slice 0
    is slice 1's first, that of slice 1 wraps to row 0."""
    f = X // m
    assert _slices(m) == slices
    vel, _ = _case(100 + X, B, X, m, NS)
    vort, vx, vy = _run(be, vel, m)
    lx = float(np.float32(TWO_PI))      # the lengths as the C ABI takes them
    u_c, v_c = co.coarsen_velocity(vel[..., 1], vel[..., 2], m)
    w_c = co.curl(u_c, v_c, lx, lx)
    for name, got, want, src in (("vx", vx, u_c, vel[..., 1]), ("vy", vy, v_c, vel[..., 2])):
        bound = f * U * np.abs(src).max()
        err = np.abs(got[T].astype(np.float64) - want).max()
        print(f"X={X} m={m} f={f}: max |{name} - float64| {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    bound = 8 * f * U * (np.abs(vel[..., 2]).max() / (lx / m) + np.abs(vel[..., 1]).max() / (lx / m))
    err = np.abs(vort[T].astype(np.float64) - w_c).max()
    print(f"X={X} m={m} f={f}: max |vort - float64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    _untouched((vort, vx, vy), T)


def test_export_takes_the_two_domain_lengths_in_their_places(be):
    vel, _ = _case(7, B, 16, 8, NS)
    vort = _run(be, vel, 8, lx=1.0, ly=3.0)[0][T].astype(np.float64)
    want = co.coarsen_from_velocity(vel, 8, 1.0, 3.0)
    bound = 8 * 2 * U * (np.abs(vel[..., 2]).max() / (1.0 / 8) + np.abs(vel[..., 1]).max() / (3.0 / 8))
    assert np.abs(vort - want).max() <= bound
    assert np.abs(vort - co.coarsen_from_velocity(vel, 8, 3.0, 1.0)).max() > 1e-2      # exchanged: far outside


def test_export_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    a, o = be.zeros((16 * 16 * 3,)), [be.zeros((2 * 16 * 16,)) for _ in range(3)]

    def step(vel, vort, vx, vy, X, Y, m, n_steps, t, B=1, lx=1.0, ly=1.0):
        return lib.ffno_prediction_export_step(vel, vort, vx, vy, B, X, Y, m, n_steps, t, lx, ly, None)

    ok = (p(a), p(o[0]), p(o[1]), p(o[2]))
    assert step(*ok, 16, 16, 8, 2, 1) == 0 and step(*ok, 16, 16, 16, 2, 0) == 0
    for k in range(4):      # each pointer null in turn
        assert step(*[None if i == k else q for i, q in enumerate(ok)], 16, 16, 8, 2, 0) == -1
    assert step(*ok, 16, 16, 8, 2, 0, B=0) == -1
    assert step(*ok, 0, 16, 8, 2, 0) == -1 and step(*ok, 16, 0, 8, 2, 0) == -1
    assert step(*ok, 16, 16, 0, 2, 0) == -1 and step(*ok, 16, 16, -8, 2, 0) == -1
    assert step(*ok, 16, 16, 8, 0, 0) == -1
    assert step(*ok, 16, 16, 8, 2, 2) == -1 and step(*ok, 16, 16, 8, 2, -1) == -1      # t outside [0, n_steps)
    assert step(*ok, 16, 16, 8, 2, 0, lx=0.0) == -1 and step(*ok, 16, 16, 8, 2, 0, ly=-1.0) == -1
    assert step(*ok, 16, 16, 6, 2, 0) == -2      # X % m
    assert step(*ok, 16, 12, 8, 2, 0) == -2      # Y % m
    assert step(*ok, 16, 8, 4, 2, 0) == -2       # X / m != Y / m
    assert step(*ok, 16, 16, 32, 2, 0) == -2     # m > X
    assert step(*ok, 8192, 8192, 8192, 2, 0) == -2      # m above the LDS limit of 4096 (refused before anything is read)
