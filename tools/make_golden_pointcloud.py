#!/usr/bin/env python3
"""Golden data for the elasticity F-FNO from the REAL reference modules (build machine only; needs a reference checkout).

Loads the reference's ``modules/iphi.py`` and ``modules/factorized_fno/point_cloud_2d.py`` on the CPU and writes
tests/golden/pointcloud_ref.npz: the state-dict names / shapes / dtypes of IPhi and of FNOFactorizedPointCloud2D (n_layers 3,
share_weight False and True), and -- at the small shape of tests/test_pointcloud_model.py -- the reference's own seeded weights,
the inputs, and its fp32 outputs, loss and parameter gradients.  Only data is written; nothing of the reference's text.

Two obstacles, both handled here without touching the checkout:
  * the reference's package ``__init__`` files import Lightning / hydra: synthetic parent packages (``__path__`` only) are
    registered first, so just the two module files and what they import (grid_2d, feedforward, linear; torch + einops) load;
  * ``IPhi.__init__`` builds its two constant tensors with ``device="cuda"``: that keyword is dropped while it is constructed.

Usage:  python tools/make_golden_pointcloud.py /path/to/reference      (or FFNO_REFERENCE=/path/to/reference)
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
    sys.exit("usage: python tools/make_golden_pointcloud.py /path/to/reference   (or FFNO_REFERENCE=...)")
OUT = os.path.join(ROOT, "tests", "golden", "pointcloud_ref.npz")

B, W, M1, M2, S1, S2, N, IPHI_W, N_LAYERS = 2, 32, 4, 3, 10, 12, 37, 16, 3


def reference_classes():
    for name, rel in (("fourierflow", "fourierflow"), ("fourierflow.modules", "fourierflow/modules"),
                      ("fourierflow.modules.factorized_fno", "fourierflow/modules/factorized_fno")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    iphi = importlib.import_module("fourierflow.modules.iphi")
    pc = importlib.import_module("fourierflow.modules.factorized_fno.point_cloud_2d")
    return iphi.IPhi, pc.FNOFactorizedPointCloud2D


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
    arrays.update(xy=xy, rr=rr, sigma=sigma,
                  shape=np.array([B, W, M1, M2, S1, S2, N, IPHI_W, N_LAYERS]))
    for tag, share in (("plain", False), ("shared", True)):
        torch.manual_seed(11 + int(share))
        model = Model(M1, M2, W, 2, 1, n_layers=N_LAYERS, s1=S1, s2=S2, share_weight=share)
        with no_device_keyword():
            iphi = IPhi(IPHI_W)
        for mod in (model, iphi):      # weights with 8 significant bits: same distribution, and the file compresses to half
            with torch.no_grad():
                for p in mod.parameters():
                    r = torch.view_as_real(p) if p.is_complex() else p
                    r.copy_(r.to(torch.bfloat16).to(torch.float32))
        if share:      # everything but the shared Fourier weights is the plain model's, so that only those are stored again
            keep = {k: v for k, v in plain_sd.items() if "fourier_weight" not in k}
            assert not model.load_state_dict(keep, strict=False).unexpected_keys
            iphi.load_state_dict(plain_iphi_sd)
        else:
            plain_sd = {k: v.clone() for k, v in model.state_dict().items()}
            plain_iphi_sd = {k: v.clone() for k, v in iphi.state_dict().items()}
        for who, mod in (("model", model), ("iphi", iphi)):
            names, shapes, dtypes = describe(mod.state_dict())
            arrays[f"{tag}.{who}.names"], arrays[f"{tag}.{who}.shapes"], arrays[f"{tag}.{who}.dtypes"] = names, shapes, dtypes
        out = model(torch.tensor(xy), code=torch.tensor(rr), iphi=iphi)
        loss = rel_l2_loss(out, torch.tensor(sigma))
        loss.backward()
        arrays[f"{tag}.out"] = out.detach().numpy()
        arrays[f"{tag}.loss"] = np.float32(loss.item())
        # the plain model carries everything; the shared one only what differs (the shared Fourier weights and their gradients)
        for who, mod in (("model", model), ("iphi", iphi)):
            for k, v in mod.state_dict().items():
                if tag == "plain" or k.startswith("fourier_weight"):
                    arrays[f"{tag}.{who}.w.{k}"] = v.detach().numpy()
            for k, p in mod.named_parameters():
                if tag == "shared" and "fourier_weight" not in k:
                    continue
                if p.grad is not None:
                    g = p.grad
                    arrays[f"{tag}.{who}.g.{k}"] = (torch.view_as_real(g) if g.is_complex() else g).numpy()
                else:
                    arrays[f"{tag}.{who}.nograd.{k}"] = np.zeros(0, np.float32)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
