#!/usr/bin/env python3
"""Golden data for the Navier-Stokes generator from the REAL reference modules (build machine only; needs a reference checkout).

Loads the reference's ``builders/synthetic/ns_2d.py`` and ``random_fields.py`` on the CPU (by file: the package ``__init__`` files
above them import h5py / Lightning / jax) and writes tests/golden/ns2d_ref.npz: at N = 16, B = 3, 10 steps of 1e-2 with two
snapshots, the reference's fp32 solutions and force fields for the forces li, kolmogorov, none and random, each with a scalar and a
per-sample viscosity, from one white-noise-plus-GaussianRF initial vorticity; and one seeded ``GaussianRF.sample``.  Before every
solver call numpy is seeded with NUMPY_SEED (the reference draws the seed of its random force from numpy).  Only data is written;
nothing of the reference's text.

Usage:  python tools/make_golden_ns2d.py /path/to/reference      (or FFNO_REFERENCE=/path/to/reference)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FFNO_REFERENCE")
SYN = os.path.join(REF or "", "fourierflow", "builders", "synthetic")
if not REF or not os.path.isfile(os.path.join(SYN, "ns_2d.py")):
    sys.exit("usage: python tools/make_golden_ns2d.py /path/to/reference   (or FFNO_REFERENCE=...)")
OUT = os.path.join(ROOT, "tests", "golden", "ns2d_ref.npz")

B, N, STEPS, DT, RECORDS, CYCLES, SCALING, NUMPY_SEED, GRF_SEED = 3, 16, 10, 1e-2, 2, 2, 0.1, 4321, 17
VISC = {"scalar": 1e-3, "array": np.array([1e-3, 2e-3, 5e-4])}


def load(name):
    spec = importlib.util.spec_from_file_location(f"reference_{name}", os.path.join(SYN, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ns, rf = load("ns_2d"), load("random_fields")
    torch.manual_seed(GRF_SEED)
    grf = rf.GaussianRF(2, N, alpha=2.5, tau=7, device="cpu").sample(B)
    # white noise on top of the smooth field: the Nyquist bins carry energy
    w0 = grf + 0.3 * torch.from_numpy(np.random.default_rng(1).standard_normal((B, N, N)).astype(np.float32))
    arrays = dict(shape=np.array([B, N, STEPS, RECORDS, CYCLES, NUMPY_SEED, GRF_SEED]), dt=np.float64(DT), scaling=np.float64(SCALING),
                  grf=grf.numpy(), w0=w0.numpy(), visc_array=VISC["array"], visc_scalar=np.float64(VISC["scalar"]))
    for force in ("li", "kolmogorov", "none", "random"):
        for vname, visc in VISC.items():
            np.random.seed(NUMPY_SEED)
            sol, f = ns.solve_navier_stokes_2d(w0.clone(), visc, STEPS * DT, DT, RECORDS, CYCLES, SCALING, 0.2, ns.Force(force), False)
            assert sol.shape == (B, N, N, RECORDS)
            arrays[f"{force}.{vname}.sol"] = sol.astype(np.float32)
            if f is not None and vname == "scalar":      # (the force does not depend on the viscosity)
                arrays[f"{force}.f"] = np.asarray(f, np.float32)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
