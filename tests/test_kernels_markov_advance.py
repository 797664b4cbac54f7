"""ffno_markov_advance (include/ffno.h; the loop body of reference routines/grid_2d_markov.py:263-321 between two forward
passes) through the C ABI, on the emulator and on the GPU.

Every statement here is an equality of bits, none a tolerance:
  field, traj[..., col]  `raw = fma(out, std, mean)` is one fused multiply-add and `prev + raw` a plain fp32 add, so both equal
                         fp32(prev + fp32(fma)) evaluated in float64 and rounded once per operation -- the statement
                         ffno_markov_traj_step is held to (the float64 product of two fp32 numbers is exact, and its sum with a
                         third rounds to fp32 like the fused operation except in double-rounding ties that random data of this
                         size does not hit; the traj_step tests rest on the same argument).
  feats                  the non-vorticity channels and the normalisation are the device code of markov_features_kernel, so
                         feats equals what ffno_markov_features(accumulate = 0) makes of `field` with the same `derived`.
"""
import ctypes

import numpy as np
import pytest

from backend_util import be  # noqa: F401
from fourierflow_amd import _capi

LOW, HIGH, EPS = -0.25, 1.5, 1e-8
EXTRAS = {"position": (1, 0, 0), "position_force_mu": (1, 1, 1), "neither": (0, 0, 0)}


def _case(seed, B, M, N):
    rs = np.random.RandomState(seed)
    out = rs.standard_normal((B, M, N)).astype(np.float32)
    prev = rs.standard_normal((B, M, N)).astype(np.float32)
    force = rs.standard_normal((B, M, N)).astype(np.float32)
    mu = rs.uniform(0.1, 1.0, B).astype(np.float32)
    affine = np.array([1.7, -0.4], np.float32)
    return out, prev, force, mu, affine


def _field(out, prev, affine):
    raw = out if affine is None else (out.astype(np.float64) * np.float64(affine[0]) + np.float64(affine[1])).astype(np.float32)
    return raw if prev is None else (prev + raw).astype(np.float32)


def _derived(be, x, use_pos, d_force, d_mu, D):
    """The {mean[D], std[D]} buffer of one accumulating ffno_markov_features call on x [B, M, N] (statistics of the test's own
    making: any positive std serves) -> device handle."""
    lib, p = be.lib, be.ptr
    B, M, N = x.shape
    extra = _capi.MarkovExtra(p(d_force), p(d_mu), use_pos, 0)
    d_state, d_derived, d_part, d_out = be.zeros((2 * D + 2,)), be.zeros((2 * D,)), be.empty((256 * 32,)), be.empty((B, M, N, D))
    assert lib.ffno_markov_features(p(be.put(x)), p(d_state), p(d_derived), None, p(d_out), p(d_part), B, M, N, 1, LOW, HIGH, 0.0,
                                    EPS, 1, 1, ctypes.byref(extra), None) == 0
    return d_state, d_derived, d_part


def _features_of(be, d_field, d_state, d_derived, d_part, use_pos, d_force, d_mu, D, normalize, shape):
    lib, p = be.lib, be.ptr
    B, M, N = shape
    extra = _capi.MarkovExtra(p(d_force), p(d_mu), use_pos, 0)
    d_out = be.empty((B, M, N, D))
    assert lib.ffno_markov_features(p(d_field), p(d_state), p(d_derived), None, p(d_out), p(d_part), B, M, N, 1, LOW, HIGH, 0.0,
                                    EPS, 0, normalize, ctypes.byref(extra), None) == 0
    return be.get(d_out)


def _advance(be, shape, seed, with_affine, with_prev, kind, normalize=1, L=4, col=2, force_stack=None):
    """One launch with every output requested -> (field, traj, feats) as numpy, the expected field, and what
    ffno_markov_features makes of the field."""
    lib, p = be.lib, be.ptr
    B, M, N = shape
    out, prev, force, mu, affine = _case(seed, B, M, N)
    affine, prev = (affine if with_affine else None), (prev if with_prev else None)
    use_pos, has_f, has_mu = EXTRAS[kind]
    D = 1 + 2 * use_pos + has_f + has_mu
    stride = 1
    if has_f and force_stack is not None:      # column 3 of a [B, M, N, T'] stack, read in place
        Tp, t = force_stack
        stack = np.random.RandomState(seed + 1).standard_normal((B, M, N, Tp)).astype(np.float32)
        stack[..., t] = force
        d_stack = be.put(stack)
        f_ptr = ctypes.c_void_p((d_stack.ctypes.data if be.kind == "emu" else d_stack.data_ptr()) + 4 * t)
        stride = Tp
    d_force = be.put(force) if has_f else None      # the contiguous copy of that column: what ffno_markov_features reads
    if has_f and force_stack is None:
        f_ptr = p(d_force)
    d_mu = be.put(mu) if has_mu else None
    d_state, d_derived, d_part = _derived(be, _field(out, prev, affine) * 0.5 + 0.1, use_pos, d_force, d_mu, D)
    d_out, d_prev, d_field = be.put(out), be.put(prev), be.empty((B, M, N))
    d_traj, d_feats = be.empty((B, M, N, L)), be.empty((B, M, N, D))
    desc = _capi.MarkovAdvanceDesc(affine=p(be.put(affine)), prev=p(d_prev), traj=p(d_traj), feats=p(d_feats), derived=p(d_derived),
                                   force=f_ptr if has_f else None, mu=p(d_mu), force_stride=stride, L=L, col=col, D=D,
                                   use_position=use_pos, normalize=normalize, low=LOW, high=HIGH)
    assert lib.ffno_markov_advance(p(d_out), p(d_field), ctypes.byref(desc), B, M, N, None) == 0
    want_feats = _features_of(be, d_field, d_state, d_derived, d_part, use_pos, d_force, d_mu, D, normalize, shape)
    return be.get(d_field), be.get(d_traj), be.get(d_feats), _field(out, prev, affine), want_feats


@pytest.mark.parametrize("kind", list(EXTRAS))
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("with_affine", [False, True])
def test_advance_field_traj_and_feats_are_bit_exact(be, with_affine, with_prev, kind):
    L, col = 4, 2
    field, traj, feats, P, want_feats = _advance(be, (3, 12, 16), 21, with_affine, with_prev, kind, L=L, col=col)
    assert np.array_equal(field, P) and np.array_equal(traj[..., col], P)
    other = [k for k in range(L) if k != col]
    assert np.isnan(traj[..., other]).all()                                    # one step writes its own column only
    assert not np.isnan(want_feats).any() and np.array_equal(feats, want_feats)
    assert np.array_equal(_advance(be, (3, 12, 16), 21, with_affine, with_prev, kind, L=L, col=0)[1][..., 0], P)
    assert np.array_equal(_advance(be, (3, 12, 16), 21, with_affine, with_prev, kind, L=L, col=L - 1)[1][..., L - 1], P)


@pytest.mark.parametrize("kind", list(EXTRAS))
def test_advance_feats_without_normalisation(be, kind):
    field, _, feats, P, want_feats = _advance(be, (3, 12, 16), 22, True, True, kind, normalize=0)
    assert np.array_equal(field, P) and np.array_equal(feats, want_feats)
    assert np.array_equal(feats[..., 0], P)                                    # channel 0 is the field itself


def test_advance_reads_a_force_column_in_place(be):
    """force + t with stride T' = 5: column t of a [B, M, N, 5] stack gives what its contiguous copy gives."""
    strided = _advance(be, (3, 12, 16), 23, True, True, "position_force_mu", force_stack=(5, 3))
    plain = _advance(be, (3, 12, 16), 23, True, True, "position_force_mu")
    assert np.array_equal(strided[2], strided[4])                              # against ffno_markov_features on the copy
    assert np.array_equal(strided[2], plain[2]) and np.array_equal(strided[0], plain[0])


def test_advance_grid_stride_loop_wraps(be):
    """2 x 64 x 64 pixels on 16 workgroups of 256 threads: every thread takes two pixels."""
    field, traj, feats, P, want_feats = _advance(be, (2, 64, 64), 24, True, True, "position_force_mu", L=3, col=1)
    assert np.array_equal(field, P) and np.array_equal(traj[..., 1], P) and np.isnan(traj[..., [0, 2]]).all()
    assert np.array_equal(feats, want_feats)


@pytest.mark.parametrize("on", ["prev", "out"])
def test_advance_in_place(be, on):
    """The routine keeps one buffer for `prev` and `field`; a caller without learn_difference may update `out` itself."""
    lib, p = be.lib, be.ptr
    B, M, N, L, col = 3, 12, 16, 3, 1
    out, prev, _, _, affine = _case(25, B, M, N)
    d_out, d_prev, d_traj = be.put(out), be.put(prev), be.empty((B, M, N, L))
    d_field = d_prev if on == "prev" else d_out
    desc = _capi.MarkovAdvanceDesc(affine=p(be.put(affine)), prev=p(d_prev), traj=p(d_traj), L=L, col=col)
    assert lib.ffno_markov_advance(p(d_out), p(d_field), ctypes.byref(desc), B, M, N, None) == 0
    P = _field(out, prev, affine)
    assert np.array_equal(be.get(d_field), P) and np.array_equal(be.get(d_traj)[..., col], P)
    untouched, orig = (d_out, out) if on == "prev" else (d_prev, prev)
    assert np.array_equal(be.get(untouched), orig)


def test_advance_without_a_descriptor_copies(be):
    lib, p = be.lib, be.ptr
    out = _case(26, 3, 12, 16)[0]
    d_field = be.empty(out.shape)
    assert lib.ffno_markov_advance(p(be.put(out)), p(d_field), None, 3, 12, 16, None) == 0
    assert np.array_equal(be.get(d_field), out)


def test_advance_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    a, b = be.zeros((64,)), be.zeros((64,))
    EINVAL = -1

    def call(out=a, field=b, size=(1, 2, 2), **kw):
        desc = _capi.MarkovAdvanceDesc(**kw)
        return lib.ffno_markov_advance(p(out), p(field), ctypes.byref(desc), *size, None)

    assert call() == 0
    assert call(out=None) == EINVAL and call(field=None) == EINVAL
    for size in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        assert call(size=size) == EINVAL
    t = be.zeros((64,))
    assert call(traj=p(t), L=3, col=2) == 0
    for L, col in ((3, 3), (3, -1), (0, 0)):
        assert call(traj=p(t), L=L, col=col) == EINVAL                         # col outside [0, L)
    assert call(L=3, col=7) == 0                                               # no traj: col is not looked at
    f, d, m = be.zeros((64,)), be.put(np.ones(32, np.float32)), be.zeros((4,))
    assert call(feats=p(f), D=3, use_position=1) == 0
    assert call(feats=p(f), D=2, use_position=1) == EINVAL                     # D != 1 + 2 use_position + force + mu
    assert call(feats=p(f), D=3, use_position=1, force=p(t), force_stride=1) == EINVAL
    assert call(feats=p(f), D=5, use_position=1, force=p(t), force_stride=1, mu=p(m)) == 0
    assert call(feats=p(f), D=17, use_position=1) == EINVAL                    # D > 16
    assert call(feats=p(f), D=3, use_position=1, normalize=1) == EINVAL        # normalize without derived
    assert call(feats=p(f), D=3, use_position=1, normalize=1, derived=p(d)) == 0
    for stride in (0, -5):
        assert call(feats=p(f), D=4, use_position=1, force=p(t), force_stride=stride) == EINVAL
