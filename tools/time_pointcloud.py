"""Times of the elasticity F-FNO at its shipped shape -- batch 20 x 972 points, width 64, modes 16, latent grid 64 x 64, IPhi width
64, n_layers 4 and 24 -- against a torch-eager fp32 evaluation of the same formulas (the restatement of
tests/pointcloud_model_oracle.py, on the same GPU, in the same process): model forward, forward + backward + optimiser step, and
separately IPhi and the output head, forward and forward + backward.  The two sides alternate (--rounds rounds of --iters calls
each, after a warm-up, HIP events around each burst, median over the rounds), and the tool checks that both compute the same
result.  Run from the repository root; prints one JSON document."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch  # noqa: E402

import pointcloud_model_oracle as pmo  # noqa: E402
from fourierflow_amd import ops  # noqa: E402
from fourierflow_amd.modules import FNOFactorizedPointCloud2D, IPhi  # noqa: E402
from fourierflow_amd.routines import PointCloudExperiment  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, nargs="*", default=[4, 24])
ap.add_argument("--step-only", type=int, default=0, metavar="L",
                help="run only training steps of the L-layer model (no eager side): the process to put under a kernel trace")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, N, W, M, S, IW = 20, 972, 64, 16, 64, 64
g = torch.Generator().manual_seed(0)
xy = torch.rand(B, N, 2, generator=g).to(dev)
rr = torch.randn(B, 42, generator=g).to(dev)
sigma = torch.randn(B, N, 1, generator=g).to(dev)


if a.step_only:
    torch.manual_seed(2)
    routine = PointCloudExperiment(FNOFactorizedPointCloud2D(M, M, W, 2, 1, n_layers=a.step_only, s1=S, s2=S).to(dev),
                                   IPhi(IW).to(dev), 1000, optimizer=dict(lr=1e-3, weight_decay=1e-4))
    for _ in range(a.iters):
        loss = routine.training_step(dict(xy=xy, rr=rr, sigma=sigma))
    torch.cuda.synchronize()
    print(json.dumps(dict(steps=a.iters, n_layers=a.step_only, loss=float(loss))))
    sys.exit(0)


def burst(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def versus(ours, eager):
    for f in (ours, eager):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = ([], [])
    for _ in range(a.rounds):
        t[0].append(burst(ours, a.iters))
        t[1].append(burst(eager, a.iters))
    o, e = statistics.median(t[0]), statistics.median(t[1])
    return dict(hip_us=round(o, 1), eager_us=round(e, 1), eager_over_hip=round(e / o, 2))


def rel(x, y):
    return float((x - y).norm() / y.norm())


res = {"shape": dict(B=B, N=N, width=W, modes=M, grid=S, iphi_width=IW), "iters": a.iters, "rounds": a.rounds}

# ---- IPhi ------------------------------------------------------------------------------------------------------------------
torch.manual_seed(0)
iphi = IPhi(IW).to(dev)
isd = {k: v.detach() for k, v in iphi.state_dict().items()}
isd_g = {k: v.detach().clone().requires_grad_(True) for k, v in iphi.state_dict().items()}
gxi = torch.randn(B, N, 2, generator=g).to(dev)
with torch.no_grad():
    res["iphi_rel_l2_hip_vs_eager"] = float("%.2e" % rel(iphi(xy, rr), pmo.iphi(isd, xy, rr, IW)))


def iphi_fb():
    torch.autograd.backward(iphi(xy, rr), gxi)


def iphi_fb_eager():
    torch.autograd.backward(pmo.iphi(isd_g, xy, rr, IW), gxi)


with torch.no_grad():
    res["iphi_forward"] = versus(lambda: iphi(xy, rr), lambda: pmo.iphi(isd, xy, rr, IW))
res["iphi_forward_backward"] = versus(iphi_fb, iphi_fb_eager)

# ---- output head -----------------------------------------------------------------------------------------------------------
torch.manual_seed(1)
host = FNOFactorizedPointCloud2D(M, M, W, 2, 1, n_layers=1, s1=S, s2=S).to(dev)
t = torch.randn(B, W, N, generator=g).to(dev).requires_grad_(True)
hsd = {"bs.weight": host.bs[1].weight.reshape(W, 2), "bs.bias": host.bs[1].bias, "fc1.weight": host.fc1.weight,
       "fc1.bias": host.fc1.bias, "fc2.weight": host.fc2.weight, "fc2.bias": host.fc2.bias}
gy = torch.randn(B, N, 1, generator=g).to(dev)
with torch.no_grad():
    res["head_rel_l2_hip_vs_eager"] = float("%.2e" % rel(ops.point_head(t, xy, host.bs[1], host.fc1, host.fc2),
                                                          pmo.point_head(hsd, t, xy)))
    res["head_forward"] = versus(lambda: ops.point_head(t, xy, host.bs[1], host.fc1, host.fc2), lambda: pmo.point_head(hsd, t, xy))
res["head_forward_backward"] = versus(
    lambda: torch.autograd.backward(ops.point_head(t, xy, host.bs[1], host.fc1, host.fc2), gy),
    lambda: torch.autograd.backward(pmo.point_head(hsd, t, xy), gy))

# ---- the model ---------------------------------------------------------------------------------------------------------------
for L in a.layers:
    torch.manual_seed(2)
    model = FNOFactorizedPointCloud2D(M, M, W, 2, 1, n_layers=L, s1=S, s2=S).to(dev)
    ip = IPhi(IW).to(dev)
    cfg = dict(modes1=M, modes2=M, width=W, n_layers=L, s1=S, s2=S, iphi_width=IW)
    sd, uniq = pmo.model_state_dict(model.state_dict(), torch.float32)
    sdi, uniqi = pmo.model_state_dict(ip.state_dict(), torch.float32)
    sd, sdi = {k: v.detach().to(dev) for k, v in sd.items()}, {k: v.detach().to(dev) for k, v in sdi.items()}
    leaves = {}
    for d in (sd, sdi):
        for k in d:
            d[k] = leaves.setdefault(d[k].data_ptr(), d[k].requires_grad_(True))
    opt = torch.optim.AdamW(list(leaves.values()), lr=1e-3, weight_decay=1e-4)
    routine = PointCloudExperiment(model, ip, 1000, optimizer=dict(lr=1e-3, weight_decay=1e-4))
    batch = dict(xy=xy, rr=rr, sigma=sigma)
    with torch.no_grad():
        key = f"model_{L}_layers"
        res[key + "_rel_l2_hip_vs_eager"] = float("%.2e" % rel(model(xy, code=rr, iphi=ip), pmo.model(sd, xy, rr, iphi_sd=sdi, **cfg)))
        res[key + "_forward"] = versus(lambda: model(xy, code=rr, iphi=ip), lambda: pmo.model(sd, xy, rr, iphi_sd=sdi, **cfg))

    def eager_step():
        opt.zero_grad(set_to_none=True)
        pmo.rel_l2_loss(pmo.model(sd, xy, rr, iphi_sd=sdi, **cfg), sigma).backward()
        opt.step()

    res[key + "_train_step"] = versus(lambda: routine.training_step(batch), eager_step)
print(json.dumps(res, indent=1))
