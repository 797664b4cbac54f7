"""Per-axis non-uniform DFT of the fully factorised point-cloud F-FNO (csrc/ffno_pointaxis.h) through the C ABI:
ffno_nudft_axis_modes / ffno_nudft_axis_points / ffno_axis_modes_to_grid / ffno_grid_to_axis_modes against float64 sums written
from the formulas of include/ffno.h, held to the bands tests/test_pointcloud_nudft.py holds the 2-D kernels to (results <= 1e-5,
gradients and adjoints <= 5e-5 rel-L2).  Every output buffer starts as NaN, so an element no thread wrote fails the comparison.

Shapes: 1, 63, 64, 65 and 130 points (one point, a ragged 64-point tile, exactly one, one past it, a tile turn-over); 1, 3, 8, 9
and 32 channels (ragged 8-channel chunks, exactly one, one past it, four); modes (1, 1), (3, 2), (16, 16) and (32, 5) (the
smallest set on one ragged 8-mode slab, unequal both ways, four full slabs, the largest m1 on five slabs with a ragged last one); coordinates partly outside the unit square and near
+-100 (the exact k x mod 1 reduction); latent grids 8 with 5 modes (a Nyquist mode), 9 (odd) and 40 (the shipped one, also with a
Nyquist mode at 21), 1 to 32 channels (ragged and several 16-channel chunks; 40 rows are ten 4-row tiles, 9 rows leave a ragged one).

Worst measured figures on the emulator: modes 2.2e-7, points 1.8e-7, dxi 3.0e-7, grid results 2.1e-7, adjoint identities 5.9e-8."""
import numpy as np
import pytest

from backend_util import Backend, BACKENDS, be, rel_l2  # noqa: F401  (be is a fixture)

FWD_TOL, GRAD_TOL = 1e-5, 5e-5
POINTS = (1, 63, 64, 65, 130)
CHANNELS = (1, 3, 8, 9, 32)
MODES = ((1, 1), (3, 2), (16, 16), (32, 5))
B = 2


def _xi(n, rng):
    """fp32 coordinates on [-0.45, 1.6]^2, every fifth point moved to within 1 of +-100."""
    xi = rng.uniform(-0.45, 1.6, (B, n, 2))
    far = np.arange(n) % 5 == 2
    xi[:, far] += np.where(rng.uniform(size=(B, int(far.sum()), 2)) < 0.5, -100.0, 100.0)
    return xi.astype(np.float32).astype(np.float64)


def _wavenumbers(m1, m2):
    """(k_t, coordinate of t) for t < m2 + m1"""
    return np.concatenate([np.arange(m2), np.arange(m1)]).astype(np.float64), np.concatenate([np.zeros(m2, int), np.ones(m1, int)])


def _basis(xi, m1, m2):
    k, d = _wavenumbers(m1, m2)
    return np.exp(2j * np.pi * xi[:, :, d] * k)      # E [B, N, K]


def _cplx(shape, rng):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64).astype(np.complex128)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _c2f(z):
    """complex [..] -> float32 [.., 2]"""
    return _f32(np.stack([z.real, z.imag], axis=-1))


def _f2c(a):
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _modes(be, u, xi, m1, m2):
    Bn, C, N = u.shape
    spec = be.empty((Bn, C, m1 + m2, 2))
    assert be.lib.ffno_nudft_axis_modes(be.ptr(be.put(_f32(u))), be.ptr(be.put(_f32(xi))), be.ptr(spec), Bn, C, N, m1, m2, None) == 0
    return _f2c(be.get(spec))


def _points(be, spec, xi, m1, m2, w=None, want_out=True, dxi0=None, accumulate=0):
    Bn, C, _ = spec.shape
    N = xi.shape[1]
    out = be.empty((Bn, C, N)) if want_out else None
    dxi = None
    if w is not None:
        dxi = be.empty((Bn, N, 2)) if dxi0 is None else be.put(_f32(dxi0))
    rc = be.lib.ffno_nudft_axis_points(be.ptr(be.put(_c2f(spec))), be.ptr(be.put(_f32(xi))), be.ptr(be.put(None if w is None else _f32(w))),
                                       be.ptr(out), be.ptr(dxi), Bn, C, N, m1, m2, accumulate, None)
    assert rc == 0
    return (None if out is None else np.array(be.get(out))), (None if dxi is None else np.array(be.get(dxi)))


@pytest.mark.parametrize("m1,m2", MODES)
def test_point_kernels_against_float64_sums(be, m1, m2):
    rng = np.random.default_rng(100 + m1 + m2)
    k, d = _wavenumbers(m1, m2)
    worst = dict(modes=0.0, points=0.0, dxi=0.0, adj=0.0)
    for N in POINTS:
        xi = _xi(N, rng)
        E = _basis(xi, m1, m2)
        for C in CHANNELS:
            u = rng.standard_normal((B, C, N)).astype(np.float32).astype(np.float64)
            V = _cplx((B, C, m1 + m2), rng)
            w = rng.standard_normal((B, C, N)).astype(np.float32).astype(np.float64)
            spec = _modes(be, u, xi, m1, m2)
            ref_spec = np.einsum("bcn,bnt->bct", u, E.conj())
            out, dxi = _points(be, V, xi, m1, m2, w=w)
            ref_out = np.einsum("bct,bnt->bcn", V, E).real
            dE = np.einsum("bct,bnt->bcnt", V, E * (2j * np.pi * k)).real                   # d out / d xi_{d(t)} per mode
            ref_dxi = np.stack([np.einsum("bcn,bcnt->bn", w, dE[..., d == a]) for a in (0, 1)], axis=-1)
            assert np.isfinite(spec.real).all() and np.isfinite(spec.imag).all() and np.isfinite(out).all() and np.isfinite(dxi).all()
            e = dict(modes=rel_l2(_c2f(spec), _c2f(ref_spec)), points=rel_l2(out, ref_out), dxi=rel_l2(dxi, ref_dxi))
            # <A u, V> = <u, A^T V> over the real pairs, on the kernels' own outputs
            lhs, rhs = float((spec.real * V.real + spec.imag * V.imag).sum()), float((u * out).sum())
            e["adj"] = abs(lhs - rhs) / (np.linalg.norm(_c2f(spec)) * np.linalg.norm(_c2f(V)))
            for key, v in e.items():
                worst[key] = max(worst[key], v)
            assert e["modes"] < FWD_TOL and e["points"] < FWD_TOL and e["dxi"] < GRAD_TOL and e["adj"] < GRAD_TOL, (N, C, e)
            # the gradient-only call (no out) and the forward-only call (no dxi) give the same bits as the combined one
            out2, _ = _points(be, V, xi, m1, m2)
            _, dxi2 = _points(be, V, xi, m1, m2, w=w, want_out=False)
            np.testing.assert_array_equal(dxi2, dxi)
            np.testing.assert_array_equal(out2, out)
    print(f"[pointaxis {be.kind} m1={m1} m2={m2}] worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_dxi_accumulates_into_the_buffer(be):
    rng = np.random.default_rng(7)
    m1, m2, C, N = 3, 2, 9, 65
    xi, V = _xi(N, rng), _cplx((B, C, m1 + m2), rng)
    w = rng.standard_normal((B, C, N)).astype(np.float32)
    base = rng.standard_normal((B, N, 2)).astype(np.float32)
    _, plain = _points(be, V, xi, m1, m2, w=w, want_out=False)
    _, acc = _points(be, V, xi, m1, m2, w=w, want_out=False, dxi0=base, accumulate=1)
    np.testing.assert_array_equal(acc, plain + base)
    _, over = _points(be, V, xi, m1, m2, w=w, want_out=False, dxi0=base, accumulate=0)      # written, not added
    np.testing.assert_array_equal(over, plain)


def test_two_calls_are_bit_equal(be):
    rng = np.random.default_rng(8)
    m1, m2, C, N, S = 16, 16, 9, 130, 40
    xi, V = _xi(N, rng), _cplx((B, C, m1 + m2), rng)
    u = rng.standard_normal((B, C, N)).astype(np.float32)
    a, b = _modes(be, u, xi, m1, m2), _modes(be, u, xi, m1, m2)
    np.testing.assert_array_equal(a, b)
    a, b = _points(be, V, xi, m1, m2, w=u), _points(be, V, xi, m1, m2, w=u)
    np.testing.assert_array_equal(a[0], b[0]), np.testing.assert_array_equal(a[1], b[1])
    g = rng.standard_normal((B, S, S, C)).astype(np.float32)
    for c2r in (0, 1):
        np.testing.assert_array_equal(_to_grid(be, V, S, m1, m2, c2r), _to_grid(be, V, S, m1, m2, c2r))
        np.testing.assert_array_equal(_to_modes(be, g, m1, m2, c2r), _to_modes(be, g, m1, m2, c2r))


# ---- modes <-> the separable latent grid -------------------------------------------------------------------------------------
def _to_grid(be, spec, S, m1, m2, c2r):
    Bn, C, _ = spec.shape
    out = be.empty((Bn, S, S, C))
    assert be.lib.ffno_axis_modes_to_grid(be.ptr(be.put(_c2f(spec))), be.ptr(out), Bn, C, S, m1, m2, c2r, None) == 0
    return np.array(be.get(out))


def _to_modes(be, grid, m1, m2, c2r):
    Bn, S, _, C = grid.shape
    spec = be.empty((Bn, C, m1 + m2, 2))
    assert be.lib.ffno_grid_to_axis_modes(be.ptr(be.put(_f32(grid))), be.ptr(spec), Bn, C, S, m1, m2, c2r, None) == 0
    return _f2c(be.get(spec))


def _line(z, S, c2r):
    """[B, C, m] -> [B, C, S]: irfft(zero-padded, n = S) or the plain Re sum_j z_j exp(2 pi i j s / S)"""
    m = z.shape[-1]
    if c2r:
        full = np.zeros(z.shape[:-1] + (S // 2 + 1,), np.complex128)
        full[..., :m] = z
        return np.fft.irfft(full, n=S, axis=-1)
    return np.einsum("bcj,js->bcs", z, np.exp(2j * np.pi * np.outer(np.arange(m), np.arange(S)) / S)).real


# (S, m1, m2): S = 8 with 5 modes and S = 40 with 21 carry the Nyquist mode; 9 is odd (no Nyquist; 5 = 9 // 2 + 1 is its last mode)
GRIDS = ((8, 5, 5), (8, 2, 5), (9, 5, 4), (40, 12, 12), (40, 3, 21))


@pytest.mark.parametrize("S,m1,m2", GRIDS)
def test_grid_kernels_against_float64_sums(be, S, m1, m2):
    rng = np.random.default_rng(200 + S + m1)
    worst = dict(grid=0.0, modes=0.0, adj=0.0)
    for C in (1, 3, 9, 32):
        V = _cplx((B, C, m1 + m2), rng)
        G = rng.standard_normal((B, S, S, C)).astype(np.float32).astype(np.float64)
        col, row = G.sum(axis=1).transpose(0, 2, 1), G.sum(axis=2).transpose(0, 2, 1)       # [B, C, y], [B, C, x]
        fy, fx = np.fft.rfft(col, axis=-1)[..., :m2], np.fft.rfft(row, axis=-1)[..., :m1]
        for c2r in (0, 1):
            grid = _to_grid(be, V, S, m1, m2, c2r)
            g, h = _line(V[..., :m2], S, c2r), _line(V[..., m2:], S, c2r)
            ref_grid = (h[:, :, :, None] + g[:, :, None, :]).transpose(0, 2, 3, 1)
            spec = _to_modes(be, G, m1, m2, c2r)
            ref_spec = np.concatenate([fy, fx], axis=-1)
            if c2r:     # the adjoint of the c2r form: c_j / S, imaginary part zero at DC and Nyquist
                a = np.concatenate([np.where((np.arange(m) == 0) | (2 * np.arange(m) == S), 1.0, 2.0) / S for m in (m2, m1)])
                edge = np.concatenate([(np.arange(m) == 0) | (2 * np.arange(m) == S) for m in (m2, m1)])
                ref_spec = ref_spec * a
                ref_spec[..., edge] = ref_spec[..., edge].real
                assert (spec.imag[..., edge] == 0).all()
            assert np.isfinite(grid).all() and np.isfinite(spec.real).all() and np.isfinite(spec.imag).all()
            e = dict(grid=rel_l2(grid, ref_grid), modes=rel_l2(_c2f(spec), _c2f(ref_spec)))
            lhs, rhs = float((grid * G).sum()), float((V.real * spec.real + V.imag * spec.imag).sum())
            e["adj"] = abs(lhs - rhs) / (np.linalg.norm(grid) * np.linalg.norm(G))
            for key, v in e.items():
                worst[key] = max(worst[key], v)
            assert e["grid"] < FWD_TOL and e["modes"] < FWD_TOL and e["adj"] < GRAD_TOL, (C, c2r, e)
    print(f"[pointaxis {be.kind} S={S} m1={m1} m2={m2}] worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_refusal_codes(be):
    lib, p = be.lib, be.ptr
    C, N, m, S = 3, 37, 2, 8
    u, xi, spec, dxi = be.zeros((B, C, N)), be.zeros((B, N, 2)), be.zeros((B, C, 2 * m, 2)), be.zeros((B, N, 2))
    grid = be.zeros((B, S, S, C))
    assert lib.ffno_nudft_axis_supported(C, 32, 32) == 1 and lib.ffno_nudft_axis_supported(C, 1, 1) == 1
    assert lib.ffno_nudft_axis_supported(C, 33, 1) == 0 and lib.ffno_nudft_axis_supported(C, 1, 33) == 0
    assert lib.ffno_nudft_axis_supported(C, 0, 1) == 0 and lib.ffno_nudft_axis_supported(0, 1, 1) == 0
    assert lib.ffno_nudft_axis_modes(None, p(xi), p(spec), B, C, N, m, m, None) == -1
    assert lib.ffno_nudft_axis_modes(p(u), p(xi), p(spec), B, C, 0, m, m, None) == -1
    assert lib.ffno_nudft_axis_modes(p(u), p(xi), p(spec), B, C, N, 33, m, None) == -2
    assert lib.ffno_nudft_axis_modes(p(u), p(xi), p(spec), 65536, C, N, m, m, None) == -2
    assert lib.ffno_nudft_axis_points(p(spec), p(xi), None, None, p(dxi), B, C, N, m, m, 0, None) == -1      # dxi needs w
    assert lib.ffno_nudft_axis_points(p(spec), p(xi), None, None, None, B, C, N, m, m, 0, None) == -1        # nothing to write
    assert lib.ffno_nudft_axis_points(p(spec), p(xi), None, p(u), None, B, C, N, m, 0, 0, None) == -1
    assert lib.ffno_nudft_axis_points(p(spec), p(xi), None, p(u), None, B, C, N, m, 33, 0, None) == -2
    assert lib.ffno_nudft_axis_points(p(spec), p(xi), None, p(u), None, 65536, C, N, m, m, 0, None) == -2
    for fn, a, b in ((lib.ffno_axis_modes_to_grid, spec, grid), (lib.ffno_grid_to_axis_modes, grid, spec)):
        assert fn(None, p(b), B, C, S, m, m, 1, None) == -1
        assert fn(p(a), p(b), B, C, 0, m, m, 1, None) == -1
        assert fn(p(a), p(b), B, C, S, 33, m, 1, None) == -2
        assert fn(p(a), p(b), 65536, C, S, m, m, 1, None) == -2
        assert fn(p(a), p(b), B, C, 300, m, m, 1, None) == -2        # S > 256
        assert fn(p(a), p(b), B, 64, 256, m, m, 1, None) == -2       # S C > 8192
        assert fn(p(a), p(b), B, C, S, 6, m, 0, None) == -3          # modes > S // 2 + 1, either flag
        assert fn(p(a), p(b), B, C, S, m, 6, 1, None) == -3
