"""CornerChain (fourierflow_amd/_corner_chain.py) driven directly through the C ABI against numpy in fp64: the analysis is the
kept corners of rfftn(norm="ortho") in the mode-major layout Z[k_last]...[k'_0][b][re/im][c], the synthesis is irfftn of the
zero-padded corners, the ``fwd=False`` synthesis is the adjoint of the analysis, and the whole convolution is analysis -> per-mode
channel mix -> synthesis.

The two shapes are the smallest with every axis of another length and every mode count different (2 K <= S on the complex axes,
K_last <= S_last // 2 + 1), so any axis or mode mix-up in the geometry changes the result.

Band: rel-L2 1e-5 (the band of the stage kernels in test_plus2d.py / test_kernels_dct.py); worst measured value of the three
rel-L2 checks over both shapes: 2.0e-7 on the emulator and on the MI355X (the 3-D convolution; analysis and synthesis alone
1.0e-7 and 8.6e-8).  Adjoint identity: 1e-3 absolute on the inner products, as test_cdft_rows_forward_inverse_and_adjoint;
worst measured difference 1.2e-5 on both (the analysis / synthesis pairs and the whole convolution against its ``fwd=False`` form)."""
import functools

import numpy as np
import pytest
import torch

from backend_util import host_device, rel_l2  # noqa: F401
from fourierflow_amd import _lib
from fourierflow_amd._corner_chain import CornerChain, checked

CASES = {"2d": (2, (8, 12), (2, 3), 32), "3d": (1, (6, 8, 10), (2, 2, 3), 32)}


def _corner_index(Sp, Ks):
    """Index of the kept corners in a [B, *rfftn bins, C] spectrum: rows [0, K) and [S - K, S) of the complex axes, [0, K) of the last."""
    rows = [np.r_[0:k, s - k:s] for k, s in zip(Ks[:-1], Sp[:-1])] + [np.arange(Ks[-1])]
    return np.ix_(*rows)


def _mode_major(A):
    """complex [B, k'_0, ..., k_last, C] -> float [k_last, ..., k'_0, B, 2, C]"""
    nd = A.ndim - 2
    A = A.transpose(*range(nd, 0, -1), 0, nd + 1)
    return np.stack([A.real, A.imag], axis=-2)


def _complex(Z):
    """float [k_last, ..., k'_0, B, 2, C] -> complex [B, k'_0, ..., k_last, C]"""
    nd = Z.ndim - 3
    Zc = Z[..., 0, :].astype(np.float64) + 1j * Z[..., 1, :]
    return Zc.transpose(nd, *range(nd - 1, -1, -1), nd + 1)


def _analysis_ref(x, Sp, Ks):
    nd = len(Sp)
    F = np.fft.rfftn(x.astype(np.float64), axes=tuple(range(1, nd + 1)), norm="ortho")
    idx = _corner_index(Sp, Ks)
    return _mode_major(np.stack([F[b][idx] for b in range(x.shape[0])]))


def _synthesis_ref(Z, Sp, Ks):
    nd = len(Sp)
    Zc = _complex(Z)
    full = np.zeros((Zc.shape[0], *Sp[:-1], Sp[-1] // 2 + 1, Zc.shape[-1]), np.complex128)
    idx = _corner_index(Sp, Ks)
    for b in range(Zc.shape[0]):
        full[b][idx] = Zc[b]
    return np.fft.irfftn(full, s=Sp, axes=tuple(range(1, nd + 1)), norm="ortho")


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (fp32) and fp64 references of one shape, computed once for every test and backend."""
    B, Sp, Ks, C = CASES[name]
    rs = np.random.RandomState(len(Sp))
    modes = Ks[-1] * int(np.prod([2 * k for k in Ks[:-1]]))
    zshape = (Ks[-1], *[2 * k for k in Ks[-2::-1]], B, 2, C)
    x = rs.standard_normal((B, *Sp, C)).astype(np.float32)
    z = rs.standard_normal(zshape).astype(np.float32)
    planes = (rs.standard_normal((modes, 2, C, C)) / np.sqrt(C)).astype(np.float32)      # [mode][re/im][i][o]
    ana = _analysis_ref(x, Sp, Ks)
    syn = _synthesis_ref(z, Sp, Ks)
    W = planes[:, 0].astype(np.float64) + 1j * planes[:, 1]
    A = (ana[..., 0, :] + 1j * ana[..., 1, :]).reshape(modes, B, C)
    Y = np.einsum("mbi,mio->mbo", A, W)
    mixed = np.stack([Y.real, Y.imag], axis=-2).reshape(zshape)
    conv = _synthesis_ref(mixed, Sp, Ks)
    out = dict(x=x, z=z, planes=planes, ana=ana, syn=syn, conv=conv)
    for a in out.values():
        a.setflags(write=False)
    return out


def _chain(name, dev):
    B, Sp, Ks, C = CASES[name]
    ch = CornerChain(B, Sp, Ks, C, checked, dev)
    # the geometry the callers size their buffers by
    assert ch.modes == Ks[-1] * int(np.prod([2 * k for k in Ks[:-1]])) and ch.spec == ch.modes * B * 2 * C and ch.R == B
    assert (ch.Bv, ch.Mv, ch.Nv) == (B * int(np.prod(Sp[:-2])), Sp[-2], Sp[-1])
    assert [p.label for p in ch.passes] == (["cdft_rows"] if len(Sp) == 2 else ["cdft_rows(y)", "cdft_rows(x)"])
    assert len(ch.mid_sizes) == len(Sp) - 1 and ch.cw_floats > 0
    return ch


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)      # (a copy: the cached case is read-only)


def _empty(n, dev):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)


def _mid(ch, dev):
    return [_empty(n, dev) for n in ch.mid_sizes], _empty(ch.cw_floats, dev)


def _analysis(ch, x, dev, fwd=True):
    z = _empty(ch.spec, dev)
    mid, cw = _mid(ch, dev)
    ch.analysis(_dev(x, dev), mid, z, cw, fwd, _lib.current_stream(dev))
    return z.cpu().numpy()


def _synthesis(ch, z, dev, fwd=True):
    out = _empty(ch.B * int(np.prod(ch.Sp)) * ch.C, dev)
    mid, cw = _mid(ch, dev)
    ch.synthesis(_dev(z, dev), mid, out, cw, fwd, _lib.current_stream(dev))
    return out.cpu().numpy().reshape(ch.B, *ch.Sp, ch.C)


@pytest.mark.parametrize("name", list(CASES))
def test_analysis_is_the_kept_corners_of_rfftn(host_device, name):
    c, ch = _case(name), _chain(name, host_device)
    err = rel_l2(_analysis(ch, c["x"], host_device).reshape(c["ana"].shape), c["ana"])
    print(f"corner chain {name} analysis rel-L2 {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_synthesis_is_irfftn_of_the_zero_padded_corners(host_device, name):
    c, ch = _case(name), _chain(name, host_device)
    err = rel_l2(_synthesis(ch, c["z"], host_device), c["syn"])
    print(f"corner chain {name} synthesis rel-L2 {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_adjoint_flags_give_the_adjoint(host_device, name):
    """<analysis(x), z> == <x, synthesis-adjoint(z)>, and the same for the other pair (what the backward passes rely on)."""
    c, ch = _case(name), _chain(name, host_device)
    x, z = c["x"].astype(np.float64), c["z"].astype(np.float64)
    lhs = (_analysis(ch, c["x"], host_device).astype(np.float64) * z.ravel()).sum()
    rhs = (x * _synthesis(ch, c["z"], host_device, fwd=False)).sum()
    print(f"corner chain {name} <analysis(x), z> - <x, synthesis^T(z)> = {lhs - rhs:.3e}")
    assert abs(lhs - rhs) < 1e-3
    lhs = (_synthesis(ch, c["z"], host_device).astype(np.float64) * x).sum()
    rhs = (z.ravel() * _analysis(ch, c["x"], host_device, fwd=False)).sum()
    print(f"corner chain {name} <synthesis(z), x> - <z, analysis^T(x)> = {lhs - rhs:.3e}")
    assert abs(lhs - rhs) < 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_whole_convolution(host_device, name):
    c, ch = _case(name), _chain(name, host_device)
    dev = host_device
    scr = ch.scratch(lambda n: _empty(n, dev))
    zbuf, ybuf = _empty(ch.spec, dev), _empty(ch.spec, dev)
    out = _empty(c["x"].size, dev)
    ch.conv(_dev(c["x"], dev), out, zbuf, ybuf, _dev(c["planes"], dev), scr, True, _lib.current_stream(dev))
    err = rel_l2(out.cpu().numpy().reshape(c["conv"].shape), c["conv"])
    print(f"corner chain {name} convolution rel-L2 {err:.3e}")
    assert err < 1e-5
    assert rel_l2(zbuf.cpu().numpy().reshape(c["ana"].shape), c["ana"]) < 1e-5      # z keeps the analysed spectrum
    # <conv(x), g> == <x, conv^T(g)>: fwd=False with the transposed planes (the kernel conjugates them), g a second grid field
    g = np.random.RandomState(9).standard_normal(c["x"].shape).astype(np.float32)
    adj = _empty(c["x"].size, dev)
    planes_t = np.ascontiguousarray(c["planes"].transpose(0, 1, 3, 2))
    ch.conv(_dev(g, dev), adj, zbuf, ybuf, _dev(planes_t, dev), scr, False, _lib.current_stream(dev))
    lhs = (out.cpu().numpy().astype(np.float64) * g.ravel()).sum()
    rhs = (adj.cpu().numpy().astype(np.float64) * c["x"].ravel()).sum()
    print(f"corner chain {name} <conv(x), g> - <x, conv^T(g)> = {lhs - rhs:.3e}")
    assert abs(lhs - rhs) < 1e-3
