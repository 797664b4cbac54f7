"""IPhi kernels (csrc/ffno_iphi.h: ffno_iphi_fwd / ffno_iphi_bwd) through the C ABI against the float64 restatement of
tests/pointcloud_model_oracle.py, on the emulator and on an MI355X.

Bands: features x, y exact and angle, radius <= 1e-6; xi <= 1e-5; every parameter gradient and dcode <= 5e-5 (rel-L2).

Why the comparison is staged.  The top NeRF frequency is B_k = pi 2^(w/4 - 1): at w = 64 one ulp of atan2f moves sin(B_15 angle)
by about 0.02, so two correct fp32 evaluations of the LITERAL formula differ by more than 1e-5 (the reference op sequence in
fp32 is 4.5e-5 from float64 there, 3e-7 at w = 32, 5e-8 at w = 16).  So (a) the kernel's four features are checked on their
own, (b) everything after them is checked against the float64 oracle evaluated FROM those features, with the one rounded fp32
product B_k * feature an fp32 evaluation feeds to sin / cos, at every width, and (c) the literal float64 formula with nothing
borrowed is checked at w = 16 and 32 at 1e-5, and at w = 64 within max(1e-5, 4 x the fp32 restatement's own distance from
float64) -- the idiom of oracle_util.check_grads_at_rounding_level.

Worst measured figures at the cases with more than one weight-gradient slice (MULTI_SLICE and GPU_ONLY below), rel-L2 against
the staged float64 oracle; the bands are those above:
    xi                                emulator 4.8e-8 (GPU_ONLY cases not run), MI355X 4.9e-8
    parameter gradients               emulator 1.5e-6, MI355X 1.5e-6 (both at (32, 3, 700))
    dcode                             emulator 1.2e-6, MI355X 1.1e-6
    at (64, 20, 972), the shipped shape, MI355X only: xi 4.9e-8, gradients 6.7e-7, dcode 5.1e-7
    at (16, 2, 33000), the 64-slice cap with an empty last slice, MI355X only: xi 3.1e-8, gradients 1.3e-6, dcode 9.7e-7
    the sentinel floats behind the workspace intact, every result finite, two backward calls bit-identical: on both"""
import ctypes

import numpy as np
import pytest
import torch

import pointcloud_model_oracle as pmo
from backend_util import be, rel_l2  # noqa: F401
from fourierflow_amd import _capi

# (width, B, N): H = 64 / 128 / 256; 74, 140 and 260 points = 3, 5 and 9 tiles of 32 with a ragged last one; and 12 samples of 3
# points: one tile touches more samples than it keeps fc_code outputs for in LDS (the per-point path of the feature stage)
CASES = [(16, 2, 37), (32, 2, 70), (64, 2, 130), (16, 12, 3)]
# P = B N >= 1024: the weight gradients are summed over nsplit = min(ceil(P / 1024), 64) point slices of
# chunk = 32 ceil(ceil(P / nsplit) / 32) points (iphi_wgrad_kernel's blockIdx.y, the nsplit loop of iphi_reduce_kernel, and the
# offsets of partial / small / dcd in the workspace, which all depend on nsplit).
#   (16, 2, 530)    P = 1060: 2 slices of 544; slice 0 crosses the sample boundary, slice 1 has 516 points = 16 k-steps and a
#                   4-point masked tail; 34 feature tiles, the last with 4 points; 17 thin-layer slices
#   (32, 3, 700)    P = 2100: 3 slices of 704, the last with 692 points; H = 128: 2 x 2 weight-gradient tiles
#   (64, 2, 600)    P = 1200: 2 slices at H = 256
#   (64, 20, 972)   P = 19 440: the shipped elasticity shape, 19 slices of 1024
#   (16, 2, 33000)  P = 66 000: the cap of 64 slices; chunk 1056 and 63 * 1056 > P, so slice 63 holds no point and writes zeros
MULTI_SLICE = [(16, 2, 530), (32, 3, 700), (64, 2, 600)]
GPU_ONLY = [(64, 20, 972), (16, 2, 33000)]
CASES += MULTI_SLICE + GPU_ONLY
TAIL, SENTINEL = 4096, np.float32(-1234.5)       # floats behind the workspace the call must leave alone


def _skip_large_on_emu(be, case):
    if be.kind == "emu" and case in GPU_ONLY:
        pytest.skip("large case runs on the GPU only")


def _inputs(width, B, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 2.0, (B, N, 2)).astype(np.float32)
    near = np.hypot(x[..., 0] - pmo.CENTER, x[..., 1] - pmo.CENTER) < 0.05
    x[near] += np.float32(0.2)
    code = rng.standard_normal((B, pmo.CODE_DIM)).astype(np.float32)       # a different code per sample
    dxi = rng.standard_normal((B, N, 2)).astype(np.float32)
    sd = pmo.linear_init(pmo.iphi_shapes(width), seed + 1)
    return sd, x, code, dxi


def _params(be, handles):
    return _capi.IPhiParams(*[be.ptr(handles[n]).value for n in pmo.IPHI_NAMES])


def _forward(be, sd, x, code, width, want_acts):
    B, N = x.shape[:2]
    H = 4 * width
    hp = {n: be.put(sd[n]) for n in pmo.IPHI_NAMES}
    hx, hc = be.put(x), be.put(code)
    xi, feat = be.empty((B, N, 2)), be.empty((B * N, 4))
    acts = be.empty((4, B * N, H)) if want_acts else None
    par = _params(be, hp)
    rc = be.lib.ffno_iphi_fwd(ctypes.byref(par), be.ptr(hx), be.ptr(hc), be.ptr(xi), be.ptr(feat), be.ptr(acts), B, N, width, None)
    assert rc == 0
    return hp, par, hx, hc, xi, feat, acts


@pytest.mark.parametrize("width,B,N", CASES)
def test_iphi_forward(be, width, B, N):
    _skip_large_on_emu(be, (width, B, N))
    sd, x, code, _ = _inputs(width, B, N, 100 + width)
    assert np.hypot(x[..., 0] - pmo.CENTER, x[..., 1] - pmo.CENTER).min() >= 0.05 and x.min() >= -1.0 and x.max() <= 2.0
    assert not np.array_equal(code[0], code[1])
    _, _, _, _, xi, feat, _ = _forward(be, sd, x, code, width, False)
    xi, feat = be.get(xi).copy(), be.get(feat).copy().reshape(B, N, 4)
    assert np.isfinite(xi).all() and np.isfinite(feat).all()

    x64, c64 = torch.tensor(x, dtype=torch.float64), torch.tensor(code, dtype=torch.float64)
    sd64 = pmo.to_torch(sd, torch.float64)
    f64 = pmo.iphi_features(x64).numpy()
    np.testing.assert_array_equal(feat[..., :2], x)
    assert rel_l2(feat[..., 2], f64[..., 2]) <= 1e-6
    assert rel_l2(feat[..., 3], f64[..., 3]) <= 1e-6

    staged = pmo.iphi(sd64, x64, c64, width, feat=torch.tensor(feat, dtype=torch.float64), fp32_products=True).numpy()
    e_staged = rel_l2(xi, staged)
    literal = pmo.iphi(sd64, x64, c64, width).numpy()
    e_lit = rel_l2(xi, literal)
    print(f"[iphi w={width} B={B} N={N}] xi vs staged float64 oracle {e_staged:.2e}, vs literal float64 oracle {e_lit:.2e}")
    assert e_staged <= 1e-5
    if width <= 32:
        assert e_lit <= 1e-5
    else:
        r32 = pmo.iphi(pmo.to_torch(sd, torch.float32), torch.tensor(x), torch.tensor(code), width).numpy()
        noise = rel_l2(r32, literal)
        print(f"[iphi w={width}] the fp32 restatement's own distance from float64: {noise:.2e}")
        assert e_lit <= max(1e-5, 4 * noise)


def iphi_backward(be, par, hx, hc, feat, acts, sd, dxi, width):
    """One ffno_iphi_bwd call into fresh NaN-filled gradient buffers and a NaN-filled workspace of exactly
    ffno_iphi_bwd_ws_floats floats with TAIL sentinel floats behind it -> ({name: gradient}, dcode, the tail afterwards)."""
    B, N = dxi.shape[:2]
    hg = {n: be.empty(sd[n].shape) for n in pmo.IPHI_NAMES}
    gpar = _params(be, hg)
    dcode = be.empty((B, pmo.CODE_DIM))
    n_ws = int(be.lib.ffno_iphi_bwd_ws_floats(B, N, width))
    assert n_ws > 0
    ws0 = np.full(n_ws + TAIL, np.nan, np.float32)
    ws0[n_ws:] = SENTINEL
    ws, hd = be.put(ws0), be.put(dxi)
    rc = be.lib.ffno_iphi_bwd(ctypes.byref(par), ctypes.byref(gpar), be.ptr(hx), be.ptr(hc), be.ptr(feat), be.ptr(acts),
                              be.ptr(hd), be.ptr(dcode), be.ptr(ws), B, N, width, None)
    assert rc == 0
    return {n: be.get(hg[n]).copy() for n in pmo.IPHI_NAMES}, be.get(dcode).copy(), be.get(ws)[n_ws:].copy()


@pytest.mark.parametrize("width,B,N", CASES)
def test_iphi_backward(be, width, B, N):
    """Every result is finite (each gradient buffer and the workspace start as NaN, so a slice nobody wrote shows), and the
    sentinel floats behind the workspace survive: ffno_iphi_bwd_ws_floats covers the offsets ffno_iphi_bwd uses."""
    _skip_large_on_emu(be, (width, B, N))
    sd, x, code, dxi = _inputs(width, B, N, 200 + width)
    hp, par, hx, hc, xi, feat, acts = _forward(be, sd, x, code, width, True)
    grads, dcode, tail = iphi_backward(be, par, hx, hc, feat, acts, sd, dxi, width)
    np.testing.assert_array_equal(tail, np.full(TAIL, SENTINEL))
    assert all(np.isfinite(g).all() for g in grads.values()) and np.isfinite(dcode).all()

    sd64 = pmo.to_torch(sd, torch.float64, requires_grad=True)
    c64 = torch.tensor(code, dtype=torch.float64, requires_grad=True)
    fk = torch.tensor(be.get(feat).copy().reshape(B, N, 4), dtype=torch.float64)
    out = pmo.iphi(sd64, torch.tensor(x, dtype=torch.float64), c64, width, feat=fk, fp32_products=True)
    (out * torch.tensor(dxi, dtype=torch.float64)).sum().backward()
    worst = 0.0
    for n in pmo.IPHI_NAMES:
        e = rel_l2(grads[n], sd64[n].grad.numpy())
        worst = max(worst, e)
        assert e <= 5e-5, (n, e)
    e = rel_l2(dcode, c64.grad.numpy())
    print(f"[iphi w={width} B={B} N={N}] worst parameter gradient {worst:.2e}, dcode {e:.2e}")
    assert e <= 5e-5


def test_iphi_backward_is_deterministic_over_slices(be):
    """"deterministic, no atomics" (csrc/ffno_iphi.h) with two gradient slices: two calls on the same saved activations, each
    into fresh buffers, agree bit for bit."""
    width, B, N = MULTI_SLICE[0]
    sd, x, code, dxi = _inputs(width, B, N, 200 + width)
    hp, par, hx, hc, xi, feat, acts = _forward(be, sd, x, code, width, True)
    g1, d1, _ = iphi_backward(be, par, hx, hc, feat, acts, sd, dxi, width)
    g2, d2, _ = iphi_backward(be, par, hx, hc, feat, acts, sd, dxi, width)
    for n in pmo.IPHI_NAMES:
        np.testing.assert_array_equal(g1[n], g2[n], err_msg=n)
    np.testing.assert_array_equal(d1, d2)


def test_iphi_is_deterministic_and_rejects(be):
    width, B, N = 16, 2, 37
    sd, x, code, _ = _inputs(width, B, N, 5)
    a = be.get(_forward(be, sd, x, code, width, False)[4]).copy()
    hp, par, hx, hc, xi, feat, _ = _forward(be, sd, x, code, width, False)
    np.testing.assert_array_equal(a, be.get(xi))
    lib, p = be.lib, be.ptr
    assert lib.ffno_iphi_supported(16) == 1 and lib.ffno_iphi_supported(64) == 1 and lib.ffno_iphi_supported(48) == 0
    assert lib.ffno_iphi_fwd(ctypes.byref(par), p(hx), p(hc), p(xi), None, None, B, N, 48, None) == -2
    assert lib.ffno_iphi_fwd(ctypes.byref(par), None, p(hc), p(xi), None, None, B, N, width, None) == -1
    assert lib.ffno_iphi_fwd(None, p(hx), p(hc), p(xi), None, None, B, N, width, None) == -1
    assert lib.ffno_iphi_bwd(ctypes.byref(par), ctypes.byref(par), p(hx), p(hc), p(feat), None, p(xi), p(xi), p(xi), B, N, width,
                             None) == -1           # no saved activations
    assert lib.ffno_iphi_bwd_ws_floats(B, N, 48) == 0
