"""One spectral layer's branch pair (reference grid_2d.py:51-99) composed from the batched GEMMs of csrc/bgemm.hip the way
engine_wide.py composes it -- truncated DFT per axis, per-mode block mix, zero-padded inverse, their adjoints through transposed
strides, the Fourier-weight gradient through split-K and the fold -- against oracle.ffno_oracle.forward_fourier: forward < 1e-5,
dx / dWr / dWi against fp64 autograd through the oracle < 5e-5 (the project's parity bars).  CPU wave emulator and MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from backend_util import be, rel_l2  # noqa: F401
from oracle import ffno_oracle as orc
from test_kernels_bgemm import make_desc


def run(be, name, ds, part=None):
    rc = be.lib.ffno_bgemm(ctypes.byref(ds), None) if part is None else be.lib.ffno_bgemm_splitk(ctypes.byref(ds), be.ptr(part), None)
    assert rc == 0, name


def spectral_pair(be, x, wy, wx, K, gy):
    """-> y, dx, dwy, dwx, the mixed spectrum of the last-axis branch [B M][K][2][C]."""
    from fourierflow_amd.engine_wide import dft_tables
    lib = be.lib
    B, M, N, C = x.shape
    X, GY = be.put(x), be.put(gy)
    S, GX = be.empty((B, M, N, C)), be.empty((B, M, N, C))
    # (weight, axis length, lines, G0, G1, (row, batch-0, batch-1) strides of a line's [L x C] image)
    axes = [(wy, N, B * M, B * M, 1, (C, N * C, 0)), (wx, M, B * N, N, B, (N * C, C, M * N * C))]
    kc = 2 * K * C
    grads, mixed = [], None
    for i, (w, L, R, G0, G1, (rs, s0, s1)) in enumerate(axes):
        F, Fi = (be.put(t) for t in dft_tables(L, K))
        Wb = be.empty((K, 2 * C, 2 * C))
        assert lib.ffno_bgemm_pack_fw(be.ptr(be.put(w)), be.ptr(Wb), C, K, None) == 0
        SP, SM, SD = be.empty((R, kc)), be.empty((R, kc)), be.empty((R, kc))
        img, spec = (rs, 1, s0, s1), (C, 1, kc, G0 * kc)
        mode = ((kc, 1, 2 * C), (2 * C, 1, 4 * C * C), (kc, 1, 2 * C))
        run(be, "dft", make_desc(be, F, X, SP, 2 * K, C, L, (L, 1), img, spec, G0, G1))
        run(be, "mix", make_desc(be, SP, Wb, SM, R, 2 * C, 2 * C, *mode, G0=K))
        run(be, "idft", make_desc(be, Fi, SM, S, L, C, 2 * K, (2 * K, 1), spec, img, G0, G1, accumulate=i))
        if i == 0:
            mixed = np.array(be.get(SM), copy=True).reshape(R, K, 2, C)
        # adjoints: transposed strides of the same tables and packs
        run(be, "idft_adj", make_desc(be, Fi, GY, SD, 2 * K, C, L, (1, 2 * K), img, spec, G0, G1))
        GW, dw = be.empty((K, 2 * C, 2 * C)), be.empty((C, C, K, 2))
        ds = make_desc(be, SP, SD, GW, 2 * C, 2 * C, R, (1, kc, 2 * C), (kc, 1, 2 * C), (2 * C, 1, 4 * C * C), G0=K)
        run(be, "fw_grad", ds, be.empty(lib.ffno_bgemm_splitk_ws_floats(ctypes.byref(ds))))
        assert lib.ffno_bgemm_fold_fw(be.ptr(GW), be.ptr(dw), C, K, 0, None) == 0
        grads.append(np.array(be.get(dw), copy=True))
        run(be, "mix_adj", make_desc(be, SD, Wb, SM, R, 2 * C, 2 * C, (kc, 1, 2 * C), (1, 2 * C, 4 * C * C), (kc, 1, 2 * C), G0=K))
        run(be, "dft_adj", make_desc(be, F, SM, GX, L, C, 2 * K, (1, L), spec, img, G0, G1, accumulate=i))
    return np.asarray(be.get(S)), np.asarray(be.get(GX)), grads[0], grads[1], mixed


@pytest.mark.parametrize("C,B,M,N,K", [(96, 2, 10, 12, 3), (96, 2, 10, 12, 5), (128, 1, 8, 8, 4)])
def test_wide_spectral_pair_vs_oracle(be, C, B, M, N, K):
    rs = np.random.RandomState(C + K)
    x = rs.standard_normal((B, M, N, C)).astype(np.float32)
    std = np.sqrt(2.0 / (2 * C * K * 2))
    wy, wx = ((rs.standard_normal((C, C, K, 2)) * std).astype(np.float32) for _ in range(2))
    gy = rs.standard_normal((B, M, N, C)).astype(np.float32)
    y, dx, dwy, dwx, mixed = spectral_pair(be, x, wy, wx, K, gy)
    ref = orc.forward_fourier(torch.tensor(x), torch.tensor(wy), torch.tensor(wx), K)
    assert rel_l2(y, ref.numpy()) < 1e-5
    # the C2R rule: the mixed DC bin has an imaginary part (complex weights), and irfft ignores it -- so does the inverse table
    assert np.abs(mixed[:, 0, 1, :]).max() > 1e-3
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wy, wx)]
    orc.forward_fourier(t[0], t[1], t[2], K).backward(torch.tensor(gy, dtype=torch.float64))
    assert rel_l2(dx, t[0].grad.numpy()) < 5e-5
    for got, want, name in ((dwy, t[1].grad.numpy(), "w_y"), (dwx, t[2].grad.numpy(), "w_x")):
        assert rel_l2(got[..., 0], want[..., 0]) < 5e-5, ("dWr", name)
        assert rel_l2(got[..., 1], want[..., 1]) < 5e-5, ("dWi", name)
