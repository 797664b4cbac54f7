#!/usr/bin/env python3
"""Golden data for the fully factorised point-cloud F-FNO from the REAL reference modules (build machine only; needs a
reference checkout with torch, numpy and einops).

Loads the reference's ``modules/iphi.py`` and ``modules/factorized_fno/mesh_plus_2d.py`` on the CPU the way
tools/make_golden_pointcloud_geofno.py does (synthetic parent packages; ``device="cuda"`` stripped while IPhi is constructed)
and writes tests/golden/pointcloud_fullyfact_ref.npz: the state-dict names / shapes / dtypes of
FNOFullyFactorizedMesh2D at n_layers 2 and 4 and of IPhi, and -- at the small shape of
tests/test_pointcloud_fullyfact_model.py -- the reference's own seeded weights, the inputs, and its fp32 output, loss and
parameter gradients.  Only data is written; nothing of the reference's text.

Usage:  python tools/make_golden_pointcloud_fullyfact.py /path/to/reference      (or FFNO_REFERENCE=/path/to/reference)
"""
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FFNO_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "fourierflow", "modules")):
    sys.exit("usage: python tools/make_golden_pointcloud_fullyfact.py /path/to/reference   (or FFNO_REFERENCE=...)")
OUT = os.path.join(ROOT, "tests", "golden", "pointcloud_fullyfact_ref.npz")

B, W, M1, M2, S, N, IPHI_W, N_LAYERS = 2, 32, 3, 2, 8, 37, 16, 2
LAYOUT_LAYERS = (2, 4)


def reference_classes():
    for name, rel in (("fourierflow", "fourierflow"), ("fourierflow.modules", "fourierflow/modules"),
                      ("fourierflow.modules.factorized_fno", "fourierflow/modules/factorized_fno")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    iphi = importlib.import_module("fourierflow.modules.iphi")
    pc = importlib.import_module("fourierflow.modules.factorized_fno.mesh_plus_2d")
    return iphi.IPhi, pc.FNOFullyFactorizedMesh2D


@contextlib.contextmanager
def no_device_keyword():
    real = {n: getattr(torch, n) for n in ("tensor", "arange")}

    def strip(fn):
        def wrapped(*a, **kw):
            kw.pop("device", None)
            return fn(*a, **kw)
        return wrapped
    for n, fn in real.items():
        setattr(torch, n, strip(fn))
    try:
        yield
    finally:
        for n, fn in real.items():
            setattr(torch, n, fn)


def rel_l2_loss(pred, target):      # LpLoss(size_average=True) on [B, -1]
    b = pred.shape[0]
    d = (pred.reshape(b, -1) - target.reshape(b, -1)).norm(dim=1)
    return (d / target.reshape(b, -1).norm(dim=1)).mean()


def describe(sd):
    return (np.array(list(sd.keys())), np.array([",".join(map(str, v.shape)) for v in sd.values()]),
            np.array([str(v.dtype) for v in sd.values()]))


def main():
    IPhi, Model = reference_classes()
    arrays = {}
    rng = np.random.default_rng(0)
    xy = rng.uniform(0.05, 0.95, (B, N, 2)).astype(np.float32)
    rr = rng.standard_normal((B, 42)).astype(np.float32)
    sigma = rng.standard_normal((B, N, 1)).astype(np.float32)
    arrays.update(xy=xy, rr=rr, sigma=sigma, shape=np.array([B, W, M1, M2, S, N, IPHI_W, N_LAYERS]),
                  layout_layers=np.array(LAYOUT_LAYERS))
    for L in LAYOUT_LAYERS:
        names, shapes, dtypes = describe(Model(M1, M2, W, 2, 1, n_layers=L, s1=S, s2=S).state_dict())
        arrays[f"layout{L}.names"], arrays[f"layout{L}.shapes"], arrays[f"layout{L}.dtypes"] = names, shapes, dtypes
    torch.manual_seed(23)
    model = Model(M1, M2, W, 2, 1, n_layers=N_LAYERS, s1=S, s2=S)
    with no_device_keyword():
        iphi = IPhi(IPHI_W)
    for mod in (model, iphi):      # weights with 8 significant bits: same distribution, and the file compresses to half
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(p.to(torch.bfloat16).to(torch.float32))
    names, shapes, dtypes = describe(iphi.state_dict())
    arrays["iphi.names"], arrays["iphi.shapes"], arrays["iphi.dtypes"] = names, shapes, dtypes
    out = model(torch.tensor(xy), code=torch.tensor(rr), iphi=iphi)
    loss = rel_l2_loss(out, torch.tensor(sigma))
    loss.backward()
    arrays["out"] = out.detach().numpy()
    arrays["loss"] = np.float32(loss.item())
    for who, mod in (("model", model), ("iphi", iphi)):
        for k, v in mod.state_dict().items():
            arrays[f"{who}.w.{k}"] = v.detach().numpy()
        for k, p in mod.named_parameters():
            if p.grad is not None:
                arrays[f"{who}.g.{k}"] = p.grad.numpy()
            else:
                arrays[f"{who}.nograd.{k}"] = np.zeros(0, np.float32)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
