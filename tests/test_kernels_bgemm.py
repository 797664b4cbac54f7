"""Batched strided fp32 GEMM family (fourierflow_amd/csrc/bgemm.hip: ffno_bgemm*) through the C ABI vs fp64 numpy: the kernels
the wide F-FNO block (widths 96 .. 256) is composed from.  Shapes are the ones at which tiling can go wrong (tile edges of the
32 / 64 / 128 variants, K chunks of 32, the split-K slice turn-over), not workload shapes.  The bar is that of
test_kernels_glin.py for the same instruction (v_mfma_f32_32x32x2_f32).  CPU wave emulator (-m "not gpu") and MI355X (-m gpu)."""
import ctypes

import numpy as np
import pytest

from backend_util import be, rel_l2  # noqa: F401

TOL = 1e-5


def make_desc(be, A, B, D, M, N, K, a, b, d, G0=1, G1=1, bias=None, gate=None, resid=None, alpha=1.0, relu=0, accumulate=0):
    """a / b / d = (row stride, column stride[, batch-0 stride, batch-1 stride]) in floats."""
    from fourierflow_amd._capi import BgemmDesc
    ds = BgemmDesc()
    for name, h in (("A", A), ("B", B), ("D", D), ("bias", bias), ("gate", gate), ("resid", resid)):
        setattr(ds, name, None if h is None else be.ptr(h).value)
    for t, s in (("a", a), ("b", b), ("d", d)):
        s = tuple(s) + (0,) * (4 - len(s))
        for f, v in zip(("rs", "cs", "g0", "g1"), s):
            setattr(ds, f"{t}_{f}", int(v))
    ds.M, ds.N, ds.K, ds.G0, ds.G1 = M, N, K, G0, G1
    ds.alpha, ds.relu, ds.accumulate = alpha, relu, accumulate
    ds.keep = (A, B, D, bias, gate, resid)      # the descriptor holds raw addresses: the operands live as long as it does
    return ds


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def f64(a):
    return np.asarray(a, np.float64)


SIZES = [1, 31, 33, 127, 129, 130]
KS = [1, 31, 32, 33, 100]


@pytest.mark.parametrize("M", SIZES)
def test_bgemm_tile_edges(be, M):
    """Every (M, N) of the edge sizes, every K against every M and every N at least once; row-major operands."""
    rs = np.random.RandomState(M)
    cases = [(N, KS[(i + SIZES.index(M)) % 5]) for i, N in enumerate(SIZES)]
    cases += [(130, K) for K in KS] if M in (33, 129) else []
    for N, K in cases:
        A, B = rnd(rs, M, K), rnd(rs, K, N)
        D = be.empty((M, N))
        ds = make_desc(be, be.put(A), be.put(B), D, M, N, K, (K, 1), (N, 1), (N, 1))
        assert be.lib.ffno_bgemm_supported(ctypes.byref(ds)) == 1
        assert be.lib.ffno_bgemm(ctypes.byref(ds), None) == 0
        assert rel_l2(be.get(D), f64(A) @ f64(B)) < TOL, (M, N, K)


@pytest.mark.parametrize("M,N,K", [(132, 36, 40), (130, 33, 33), (33, 130, 100)])
def test_bgemm_transposed_operands_through_strides(be, M, N, K):
    """A stored [K][M] and B stored [N][K]: the transposes live in the strides (16-byte row-wise staging when M / K allow it,
    4-byte otherwise)."""
    rs = np.random.RandomState(M + N + K)
    At, Bt = rnd(rs, K, M), rnd(rs, N, K)
    D = be.empty((M, N))
    ds = make_desc(be, be.put(At), be.put(Bt), D, M, N, K, (1, M), (1, K), (N, 1))
    assert be.lib.ffno_bgemm(ctypes.byref(ds), None) == 0
    assert rel_l2(be.get(D), f64(At).T @ f64(Bt).T) < TOL
    # ... and a transposed D (column stride M)
    Dt = be.empty((N, M))
    ds = make_desc(be, be.put(At), be.put(Bt), Dt, M, N, K, (1, M), (1, K), (1, M))
    assert be.lib.ffno_bgemm(ctypes.byref(ds), None) == 0
    assert rel_l2(be.get(Dt), (f64(At).T @ f64(Bt).T).T) < TOL


@pytest.mark.parametrize("G1,G0", [(2, 3), (4, 16)], ids=["6_products", "64_products"])
def test_bgemm_two_level_batch_shared_operand_and_padded_rows(be, G1, G0):
    """G1 x G0 products; A is shared along level 0 (stride 0); the rows of D are 7 floats longer than N (the pad keeps its NaN)."""
    rs = np.random.RandomState(5)
    M, N, K, ld = 33, 37, 35, 44
    A, B = rnd(rs, G1, M, K), rnd(rs, G1, G0, K, N)
    D = be.empty((G1, G0, M, ld))
    ds = make_desc(be, be.put(A), be.put(B), D, M, N, K, (K, 1, 0, M * K), (N, 1, K * N, G0 * K * N), (ld, 1, M * ld, G0 * M * ld),
                   G0=G0, G1=G1)
    assert be.lib.ffno_bgemm(ctypes.byref(ds), None) == 0
    out = np.asarray(be.get(D))
    ref = np.einsum("gmk,ghkn->ghmn", f64(A), f64(B))
    assert rel_l2(out[..., :N], ref) < TOL
    assert np.isnan(out[..., N:]).all()


EPI = ["none", "alpha", "bias", "relu", "gate", "resid", "accumulate", "all"]


@pytest.mark.parametrize("opt", EPI)
def test_bgemm_epilogue(be, opt):
    rs = np.random.RandomState(11)
    M, N, K = 70, 130, 33
    A, B = rnd(rs, M, K), rnd(rs, K, N)
    bias, gate, resid = rnd(rs, N), rnd(rs, M, N), rnd(rs, M, N)
    on = lambda name: opt in (name, "all")      # noqa: E731
    alpha = 0.37 if on("alpha") else 1.0
    D = be.put(np.ones((M, N), np.float32))     # accumulate: onto ones
    ds = make_desc(be, be.put(A), be.put(B), D, M, N, K, (K, 1), (N, 1), (N, 1), alpha=alpha, relu=int(on("relu")),
                   bias=be.put(bias) if on("bias") else None, gate=be.put(gate) if on("gate") else None,
                   resid=be.put(resid) if on("resid") else None, accumulate=int(on("accumulate")))
    assert be.lib.ffno_bgemm(ctypes.byref(ds), None) == 0
    ref = alpha * (f64(A) @ f64(B))
    if on("bias"):
        ref = ref + f64(bias)
    if on("relu"):
        ref = np.maximum(ref, 0)
    if on("gate"):
        ref = ref * (gate > 0)
    if on("resid"):
        ref = ref + f64(resid)
    if on("accumulate"):
        ref = ref + 1.0
    assert rel_l2(be.get(D), ref) < TOL


@pytest.mark.parametrize("K", [4096, 4097, 8193])
def test_bgemm_splitk_and_colsum_are_exact_and_bit_reproducible(be, K):
    """Weight-gradient shape: X^T . G over K rows (A through transposed strides), where the slice count turns over and where the
    last slice holds one row; the column sum of G at the same K.  Accumulate onto ones; two calls bit-identical."""
    lib = be.lib
    rs = np.random.RandomState(K)
    M, N = 33, 31
    X, G = rnd(rs, K, M), rnd(rs, K, N)
    dX, dG = be.put(X), be.put(G)
    outs = []
    for _ in range(2):
        D = be.put(np.ones((M, N), np.float32))
        ds = make_desc(be, dX, dG, D, M, N, K, (1, M), (N, 1), (N, 1), accumulate=1)
        n = lib.ffno_bgemm_splitk_slices(ctypes.byref(ds))
        assert n >= (K + 4095) // 4096 and lib.ffno_bgemm_splitk_ws_floats(ctypes.byref(ds)) == n * M * N
        part = be.empty(n * M * N)
        assert lib.ffno_bgemm_splitk(ctypes.byref(ds), be.ptr(part), None) == 0
        outs.append(np.array(be.get(D), copy=True))
    assert rel_l2(outs[0], f64(X).T @ f64(G) + 1.0) < TOL
    assert np.array_equal(outs[0], outs[1])
    # one more row of K = one more slice exactly where the previous slice was full
    ds1 = make_desc(be, dX, dG, D, M, N, K - 1, (1, M), (N, 1), (N, 1))
    if K % 4096 == 1:
        assert lib.ffno_bgemm_splitk_slices(ctypes.byref(ds1)) == n - 1
    # the same product without the split agrees to rounding
    D1 = be.empty((M, N))
    assert lib.ffno_bgemm(ctypes.byref(make_desc(be, dX, dG, D1, M, N, K, (1, M), (N, 1), (N, 1))), None) == 0
    assert rel_l2(be.get(D1), f64(X).T @ f64(G)) < TOL
    # column sum (bias gradient): 70 columns = two column chunks, rows 75 floats apart
    Nc, ld = 70, 75
    Y = rnd(rs, K, ld)
    dY = be.put(Y)
    sums = []
    for _ in range(2):
        out = be.put(np.ones(Nc, np.float32))
        nws = lib.ffno_bgemm_colsum_ws_floats(K, Nc)
        assert nws == ((K + 1023) // 1024) * Nc
        part = be.empty(nws)
        assert lib.ffno_bgemm_colsum(be.ptr(dY), ld, K, Nc, be.ptr(part), be.ptr(out), 1, None) == 0
        sums.append(np.array(be.get(out), copy=True))
    assert rel_l2(sums[0], f64(Y)[:, :Nc].sum(0) + 1.0) < TOL
    assert np.array_equal(sums[0], sums[1])


def test_bgemm_pack_and_fold_of_the_fourier_weights(be):
    """[xr | xi] . pack(w)[k] is the complex product x_k . w_k; fold is the adjoint of pack (accumulate serves share_weight)."""
    lib = be.lib
    rs = np.random.RandomState(3)
    C, K = 96, 3
    w = rnd(rs, C, C, K, 2)
    Wb = be.empty((K, 2 * C, 2 * C))
    assert lib.ffno_bgemm_pack_fw(be.ptr(be.put(w)), be.ptr(Wb), C, K, None) == 0
    Wr, Wi = w[..., 0].transpose(2, 0, 1), w[..., 1].transpose(2, 0, 1)      # [k][in][out]
    ref = np.concatenate([np.concatenate([Wr, Wi], 2), np.concatenate([-Wi, Wr], 2)], 1)
    assert np.array_equal(np.asarray(be.get(Wb)), ref)
    G = rnd(rs, K, 2 * C, 2 * C)
    g64 = f64(G)
    dre = (g64[:, :C, :C] + g64[:, C:, C:]).transpose(1, 2, 0)
    dim = (g64[:, :C, C:] - g64[:, C:, :C]).transpose(1, 2, 0)
    dref = np.stack([dre, dim], -1)
    for acc in (0, 1):
        dw = be.put(np.ones((C, C, K, 2), np.float32))
        assert lib.ffno_bgemm_fold_fw(be.ptr(be.put(G)), be.ptr(dw), C, K, acc, None) == 0
        assert rel_l2(be.get(dw), dref + acc) < 1e-6


def test_bgemm_argument_checks(be):
    lib = be.lib
    x = be.zeros((4, 4))
    ok = make_desc(be, x, x, be.zeros((4, 4)), 4, 4, 4, (4, 1), (4, 1), (4, 1))
    assert lib.ffno_bgemm_supported(ctypes.byref(ok)) == 1
    assert lib.ffno_bgemm(None, None) == -1 and lib.ffno_bgemm_supported(None) == 0
    for field in ("A", "B", "D"):
        bad = make_desc(be, x, x, be.zeros((4, 4)), 4, 4, 4, (4, 1), (4, 1), (4, 1))
        setattr(bad, field, None)
        assert lib.ffno_bgemm(ctypes.byref(bad), None) == -1
        assert lib.ffno_bgemm_splitk(ctypes.byref(bad), be.ptr(x), None) == -1
    assert lib.ffno_bgemm_splitk(ctypes.byref(ok), None, None) == -1
    bad = make_desc(be, x, x, be.zeros((4, 4)), 4, 0, 4, (4, 1), (4, 1), (4, 1))
    assert lib.ffno_bgemm(ctypes.byref(bad), None) == -1
    # every output element needs its own address: a zero stride on D is refused
    for d in ((4, 0), (0, 1)):
        bad = make_desc(be, x, x, be.zeros((4, 4)), 4, 4, 4, (4, 1), (4, 1), d)
        assert lib.ffno_bgemm(ctypes.byref(bad), None) == -2 and lib.ffno_bgemm_supported(ctypes.byref(bad)) == 0
        assert lib.ffno_bgemm_splitk_slices(ctypes.byref(bad)) == 0 and lib.ffno_bgemm_splitk_ws_floats(ctypes.byref(bad)) == 0
    bad = make_desc(be, x, x, be.zeros((4, 4)), 2, 4, 4, (4, 1), (4, 1), (4, 1), G0=2)      # two batches onto one D
    assert lib.ffno_bgemm(ctypes.byref(bad), None) == -2
    assert lib.ffno_bgemm_colsum(None, 4, 4, 4, be.ptr(x), be.ptr(x), 0, None) == -1
    assert lib.ffno_bgemm_colsum(be.ptr(x), 4, 4, 0, be.ptr(x), be.ptr(x), 0, None) == -1
    assert lib.ffno_bgemm_colsum_ws_floats(0, 4) == 0
    assert lib.ffno_bgemm_pack_fw(None, be.ptr(x), 2, 1, None) == -1
    assert lib.ffno_bgemm_fold_fw(be.ptr(x), None, 2, 1, 0, None) == -1
