"""Output head of the point-cloud F-FNO (csrc/ffno_pchead.h: ffno_pchead_fwd / ffno_pchead_bwd) through the C ABI against
the float64 restatement of tests/pointcloud_model_oracle.py, on the emulator and on an MI355X: forward <= 1e-5, dt and the
parameter gradients <= 5e-5 (rel-L2).

Worst measured figures at the cases with more than 128 tiles (MULTI_PASS below: workgroups that walk two or three tiles):
    forward                           emulator 2.8e-7, MI355X 2.8e-7
    dt and the parameter gradients    emulator 4.4e-7, MI355X 5.0e-7 (bs.bias at (64, 3, 4200, 1))
    the sentinel floats behind `partial` intact, every result finite, two backward calls bit-identical: on both"""
import ctypes

import numpy as np
import pytest
import torch

import pointcloud_model_oracle as pmo
from backend_util import be, rel_l2  # noqa: F401
from fourierflow_amd import _capi

# (W, B, N, out): both widths, one / three tiles per sample with a ragged tail, one and several output channels
CASES = [(32, 2, 37, 1), (64, 2, 130, 1), (32, 2, 70, 3)]
# More than kMaxSplit = 128 tiles of 64 points: ffno_pchead_bwd launches 128 workgroups and workgroup g walks the tiles g, g + 128,
# ..., carrying fc1's gradient in MFMA accumulators, the bias / bs sums in registers and fc2's sums in its slice of `partial`
# from tile to tile, and reusing the LDS tile buffers behind the barrier at the top of the loop.
#   (32, 3, 2757, 1)  44 tiles per sample, the last with 5 points, 132 in all: workgroups 0..3 make a second pass, on tiles of
#                     sample 2, the ragged one included
#   (64, 3, 4200, 1)  198 tiles: 70 workgroups walk two
#   (64, 5, 1700, 3)  27 tiles per sample, the last with 36 points, 135 in all; 3 outputs: 3 * 128 + 3 = 387 > 256 fc2 sums, so a
#                     thread carries more than one of them across the passes
#   (64, 20, 972, 1)  the shipped elasticity shape, 320 tiles: three passes for workgroups 0..63, two for the rest
MULTI_PASS = [(32, 3, 2757, 1), (64, 3, 4200, 1), (64, 5, 1700, 3), (64, 20, 972, 1)]
CASES += MULTI_PASS
MAX_SPLIT = 128
TAIL, SENTINEL = 4096, np.float32(-1234.5)       # floats behind `partial` the call must leave alone


def _inputs(W, B, N, out, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((B, W, N)).astype(np.float32)
    x = rng.uniform(0.0, 1.0, (B, N, 2)).astype(np.float32)
    dy = rng.standard_normal((B, N, out)).astype(np.float32)
    return pmo.linear_init(pmo.head_shapes(W, out), seed + 1), t, x, dy


def _params(be, handles):
    return _capi.PcHeadParams(*[be.ptr(handles[n]).value for n in pmo.HEAD_NAMES])


def pchead_forward(be, sd, t, x, out):
    """ffno_pchead_fwd with the saved pre-activations -> (parameter struct, device t, x, y, pre); the handles keep the buffers."""
    B, W, N = t.shape
    hp = {n: be.put(sd[n]) for n in pmo.HEAD_NAMES}
    par = _params(be, hp)
    ht, hx = be.put(t), be.put(x)
    y, pre = be.empty((B, N, out)), be.empty((B * N, 128))
    assert be.lib.ffno_pchead_fwd(ctypes.byref(par), be.ptr(ht), be.ptr(hx), be.ptr(y), be.ptr(pre), B, N, W, out, None) == 0
    return (par, hp), ht, hx, y, pre


def pchead_backward(be, par, ht, hx, pre, sd, dy):
    """One ffno_pchead_bwd call into fresh NaN-filled gradient buffers and a NaN-filled `partial` of exactly
    ffno_pchead_partial_floats floats with TAIL sentinel floats behind it -> (dt, {name: gradient}, the tail afterwards)."""
    lib, p = be.lib, be.ptr
    B, W, N = ht.shape
    out = dy.shape[2]
    hg = {n: be.empty(sd[n].shape) for n in pmo.HEAD_NAMES}
    gpar = _params(be, hg)
    dt = be.empty((B, W, N))
    n_part = int(lib.ffno_pchead_partial_floats(B, N, W, out))
    tiles = B * ((N + 63) // 64)
    assert n_part == min(tiles, MAX_SPLIT) * (128 * W + 128 + 128 * out + out + 3 * W)
    part0 = np.full(n_part + TAIL, np.nan, np.float32)
    part0[n_part:] = SENTINEL
    part, hdy = be.put(part0), be.put(dy)
    assert lib.ffno_pchead_bwd(ctypes.byref(par[0]), ctypes.byref(gpar), p(ht), p(hx), p(hdy), p(pre), p(dt), p(part), B, N, W, out,
                               None) == 0
    return be.get(dt).copy(), {n: be.get(hg[n]).copy() for n in pmo.HEAD_NAMES}, be.get(part)[n_part:].copy()


@pytest.mark.parametrize("W,B,N,out", CASES)
def test_pchead_forward_and_backward(be, W, B, N, out):
    """Every result is finite (the gradient buffers and `partial` start as NaN) and the sentinel floats behind `partial`
    survive; ffno_pchead_partial_floats is min(tiles, 128) slices of the six parameter gradients."""
    sd, t, x, dy = _inputs(W, B, N, out, 300 + W + N)
    lib, p = be.lib, be.ptr
    par, ht, hx, y, pre = pchead_forward(be, sd, t, x, out)
    y2 = be.empty((B, N, out))
    assert lib.ffno_pchead_fwd(ctypes.byref(par[0]), p(ht), p(hx), p(y2), None, B, N, W, out, None) == 0  # inference: no `pre`

    sd64 = pmo.to_torch(sd, torch.float64, requires_grad=True)
    t64 = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    ref = pmo.point_head(sd64, t64, torch.tensor(x, dtype=torch.float64))
    assert np.isfinite(be.get(y)).all()
    e = rel_l2(be.get(y), ref.detach().numpy())
    print(f"[pchead W={W} B={B} N={N} out={out}] forward {e:.2e}")
    assert e <= 1e-5
    np.testing.assert_array_equal(be.get(y), be.get(y2))

    dt, grads, tail = pchead_backward(be, par, ht, hx, pre, sd, dy)
    np.testing.assert_array_equal(tail, np.full(TAIL, SENTINEL))
    assert np.isfinite(dt).all() and all(np.isfinite(g).all() for g in grads.values())
    (ref * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    errs = {"dt": rel_l2(dt, t64.grad.numpy())}
    for n in pmo.HEAD_NAMES:
        errs[n] = rel_l2(grads[n], sd64[n].grad.numpy())
    print(f"[pchead W={W} B={B} N={N} out={out}] gradients " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 5e-5, (k, v)


def test_pchead_backward_is_deterministic_over_passes(be):
    """"deterministic, no atomics" (csrc/ffno_pchead.h) with workgroups that walk two tiles: two calls on the same saved
    pre-activations, each into fresh buffers, agree bit for bit."""
    W, B, N, out = MULTI_PASS[0]
    sd, t, x, dy = _inputs(W, B, N, out, 300 + W + N)
    par, ht, hx, y, pre = pchead_forward(be, sd, t, x, out)
    dt1, g1, _ = pchead_backward(be, par, ht, hx, pre, sd, dy)
    dt2, g2, _ = pchead_backward(be, par, ht, hx, pre, sd, dy)
    np.testing.assert_array_equal(dt1, dt2)
    for n in pmo.HEAD_NAMES:
        np.testing.assert_array_equal(g1[n], g2[n], err_msg=n)


def test_pchead_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    B = 2
    sd, t, x, _ = _inputs(32, B, 37, 1, 1)
    hp = {n: be.put(sd[n]) for n in pmo.HEAD_NAMES}
    par = _params(be, hp)
    ht, hx, y = be.put(t), be.put(x), be.empty((B, 37, 1))
    assert lib.ffno_pchead_supported(32, 128, 1) == 1 and lib.ffno_pchead_supported(64, 128, 4) == 1
    assert lib.ffno_pchead_supported(48, 128, 1) == 0 and lib.ffno_pchead_supported(32, 64, 1) == 0
    assert lib.ffno_pchead_fwd(ctypes.byref(par), p(ht), p(hx), p(y), None, B, 37, 48, 1, None) == -2
    assert lib.ffno_pchead_fwd(ctypes.byref(par), None, p(hx), p(y), None, B, 37, 32, 1, None) == -1
    assert lib.ffno_pchead_bwd(ctypes.byref(par), ctypes.byref(par), p(ht), p(hx), p(y), None, p(y), p(y), B, 37, 32, 1, None) == -1
    assert lib.ffno_pchead_partial_floats(B, 37, 48, 1) == 0
