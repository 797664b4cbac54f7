"""Per-launch time of the non-uniform DFT entry points (ffno_nudft_*) at the elasticity F-FNO shape: batch 20 x 972 points,
width 64, modes 16.  HIP-event pair around --iters back-to-back launches of each call.  For comparison it also times the same
transforms (forward, and forward + backward through autograd) as torch eager float32 on the same GPU, written the way the
reference writes fft2d / ifft2d.  Run from the repository root."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from fourierflow_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
a = ap.parse_args()
lib = _lib.get_lib()
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(0)
B, N, W, m = 20, 972, 64, 16
xi = (torch.rand(B, N, 2, generator=g) * 1.2 - 0.1).to(dev)
u3 = torch.randn(B, 3, N, generator=g).to(dev)
uW = torch.randn(B, W, N, generator=g).to(dev)
spec3 = torch.empty(B, 3, 2 * m, m, 2, device=dev)
specW = torch.randn(B, W, 2 * m, m, 2, generator=g).to(dev)
dspec = torch.empty_like(specW)
out = torch.empty(B, W, N, device=dev)
dxi = torch.zeros(B, N, 2, device=dev)
d3 = torch.empty(B, 3, N, device=dev)
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
s = torch.cuda.current_stream().cuda_stream
calls = {
    "modes C=3 (fft2d of [x,y,1])": lambda: lib.ffno_nudft_modes(P(u3), P(xi), P(spec3), B, 3, N, m, m, 0, s),
    "points C=3 + dxi (fft2d adjoint)": lambda: lib.ffno_nudft_points(P(spec3), P(xi), P(u3), P(d3), P(dxi), B, 3, N, m, m, 0, 1, s),
    "points C=64 (ifft2d)": lambda: lib.ffno_nudft_points(P(specW), P(xi), None, P(out), None, B, W, N, m, m, 1, 0, s),
    "modes C=64 quirk (ifft2d dV)": lambda: lib.ffno_nudft_modes(P(uW), P(xi), P(dspec), B, W, N, m, m, 1, s),
    "points C=64 dxi (ifft2d xi grad)": lambda: lib.ffno_nudft_points(P(specW), P(xi), P(uW), None, P(dxi), B, W, N, m, m, 1, 1, s),
}
res = {}
for name, f in calls.items():
    for _ in range(5):
        assert f() == 0, name
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    res[name] = round(e0.elapsed_time(e1) * 1000.0 / a.iters, 2)
assert torch.isfinite(out).all() and torch.isfinite(dxi).all() and torch.isfinite(dspec).all()


def _basis(x, sign):
    k1 = torch.cat((torch.arange(0, m), torch.arange(-m, 0))).reshape(2 * m, 1).repeat(1, 2 * m - 1).to(dev)
    k2 = torch.cat((torch.arange(0, m), torch.arange(-(m - 1), 0))).reshape(1, 2 * m - 1).repeat(2 * m, 1).to(dev)
    K = torch.outer(x[..., 0].reshape(-1), k1.reshape(-1).float()) + torch.outer(x[..., 1].reshape(-1), k2.reshape(-1).float())
    return torch.exp(sign * 1j * 2 * np.pi * K.reshape(B, N, 2 * m, 2 * m - 1))


def torch_fft2d(u, x):
    Y = torch.einsum("bcn,bnxy->bcxy", u + 0j, _basis(x, -1))
    return torch.cat([Y[:, :, :m, :m], Y[:, :, -m:, :m]], dim=-2)


def torch_ifft2d(V, x):
    V = torch.cat([V, V[..., 1:].flip(-1, -2).conj()], dim=-1)
    return torch.einsum("bcxy,bnxy->bcn", V, _basis(x, 1)).real


# the eager restatement computes what the launches computed (spec3 / out are the last fft2d / ifft2d results above)
lib.ffno_nudft_modes(P(u3), P(xi), P(spec3), B, 3, N, m, m, 0, s)
lib.ffno_nudft_points(P(specW), P(xi), None, P(out), None, B, W, N, m, m, 1, 0, s)
with torch.no_grad():
    agree = {"fft2d": (torch.view_as_real(torch_fft2d(u3, xi)) - spec3).norm().item() / spec3.norm().item(),
             "ifft2d": (torch_ifft2d(torch.view_as_complex(specW), xi) - out).norm().item() / out.norm().item()}
assert max(agree.values()) < 1e-4, agree
xg = xi.clone().requires_grad_(True)
u3g = u3.clone().requires_grad_(True)
Vg = torch.view_as_complex(specW.clone()).requires_grad_(True)


def fwd_bwd_fft():
    torch.autograd.grad(torch.view_as_real(torch_fft2d(u3g, xg)).sum(), (u3g, xg))


def fwd_bwd_ifft():
    torch.autograd.grad(torch_ifft2d(Vg, xg).sum(), (Vg, xg))


eager = {
    "fft2d C=3 forward": lambda: torch_fft2d(u3, xi),
    "fft2d C=3 forward + backward (du, dxi)": fwd_bwd_fft,
    "ifft2d C=64 forward": lambda: torch_ifft2d(torch.view_as_complex(specW), xi),
    "ifft2d C=64 forward + backward (dV, dxi)": fwd_bwd_ifft,
}
res_eager = {}
n_eager = max(1, a.iters // 10)
for name, f in eager.items():
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n_eager):
        f()
    e1.record()
    torch.cuda.synchronize()
    res_eager[name] = round(e0.elapsed_time(e1) * 1000.0 / n_eager, 1)
print(json.dumps({"shape": dict(B=B, N=N, W=W, modes=m), "us_per_launch": res, "torch_eager_fp32_us_per_call": res_eager,
                  "rel_l2_launch_vs_eager": {k: float("%.2e" % v) for k, v in agree.items()}},
                 indent=1))
