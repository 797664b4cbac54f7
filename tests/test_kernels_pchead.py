"""Output head of the point-cloud F-FNO (csrc/ffno_pchead.h: ffno_pchead_fwd / ffno_pchead_bwd) through the C ABI against
the float64 restatement of tests/pointcloud_model_oracle.py, on the emulator and on an MI355X: forward <= 1e-5, dt and the
parameter gradients <= 5e-5 (rel-L2)."""
import ctypes

import numpy as np
import pytest
import torch

import pointcloud_model_oracle as pmo
from backend_util import be, rel_l2  # noqa: F401
from fourierflow_amd import _capi

# (W, N, out): both widths, one / three tiles per sample with a ragged tail, one and several output channels
CASES = [(32, 37, 1), (64, 130, 1), (32, 70, 3)]
B = 2


def _inputs(W, N, out, seed):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((B, W, N)).astype(np.float32)
    x = rng.uniform(0.0, 1.0, (B, N, 2)).astype(np.float32)
    dy = rng.standard_normal((B, N, out)).astype(np.float32)
    return pmo.linear_init(pmo.head_shapes(W, out), seed + 1), t, x, dy


def _params(be, handles):
    return _capi.PcHeadParams(*[be.ptr(handles[n]).value for n in pmo.HEAD_NAMES])


@pytest.mark.parametrize("W,N,out", CASES)
def test_pchead_forward_and_backward(be, W, N, out):
    sd, t, x, dy = _inputs(W, N, out, 300 + W + N)
    lib, p = be.lib, be.ptr
    hp = {n: be.put(sd[n]) for n in pmo.HEAD_NAMES}
    par = _params(be, hp)
    ht, hx, hdy = be.put(t), be.put(x), be.put(dy)
    y, pre = be.empty((B, N, out)), be.empty((B * N, 128))
    assert lib.ffno_pchead_fwd(ctypes.byref(par), p(ht), p(hx), p(y), p(pre), B, N, W, out, None) == 0
    y2 = be.empty((B, N, out))
    assert lib.ffno_pchead_fwd(ctypes.byref(par), p(ht), p(hx), p(y2), None, B, N, W, out, None) == 0    # inference: no `pre`

    sd64 = pmo.to_torch(sd, torch.float64, requires_grad=True)
    t64 = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    ref = pmo.point_head(sd64, t64, torch.tensor(x, dtype=torch.float64))
    e = rel_l2(be.get(y), ref.detach().numpy())
    print(f"[pchead W={W} N={N} out={out}] forward {e:.2e}")
    assert e <= 1e-5
    np.testing.assert_array_equal(be.get(y), be.get(y2))

    hg = {n: be.empty(sd[n].shape) for n in pmo.HEAD_NAMES}
    gpar = _params(be, hg)
    dt = be.empty((B, W, N))
    n_part = int(lib.ffno_pchead_partial_floats(B, N, W, out))
    assert n_part > 0
    part = be.empty(n_part)
    assert lib.ffno_pchead_bwd(ctypes.byref(par), ctypes.byref(gpar), p(ht), p(hx), p(hdy), p(pre), p(dt), p(part), B, N, W, out,
                               None) == 0
    (ref * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    errs = {"dt": rel_l2(be.get(dt), t64.grad.numpy())}
    for n in pmo.HEAD_NAMES:
        errs[n] = rel_l2(be.get(hg[n]), sd64[n].grad.numpy())
    print(f"[pchead W={W} N={N} out={out}] gradients " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 5e-5, (k, v)


def test_pchead_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    sd, t, x, _ = _inputs(32, 37, 1, 1)
    hp = {n: be.put(sd[n]) for n in pmo.HEAD_NAMES}
    par = _params(be, hp)
    ht, hx, y = be.put(t), be.put(x), be.empty((B, 37, 1))
    assert lib.ffno_pchead_supported(32, 128, 1) == 1 and lib.ffno_pchead_supported(64, 128, 4) == 1
    assert lib.ffno_pchead_supported(48, 128, 1) == 0 and lib.ffno_pchead_supported(32, 64, 1) == 0
    assert lib.ffno_pchead_fwd(ctypes.byref(par), p(ht), p(hx), p(y), None, B, 37, 48, 1, None) == -2
    assert lib.ffno_pchead_fwd(ctypes.byref(par), None, p(hx), p(y), None, B, 37, 32, 1, None) == -1
    assert lib.ffno_pchead_bwd(ctypes.byref(par), ctypes.byref(par), p(ht), p(hx), p(y), None, p(y), p(y), B, 37, 32, 1, None) == -1
    assert lib.ffno_pchead_partial_floats(B, 37, 48, 1) == 0
