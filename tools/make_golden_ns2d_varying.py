#!/usr/bin/env python3
"""Golden data for the time-varying random force of the Navier-Stokes generator from the REAL reference module (build machine
only; needs a reference checkout).

Loads the reference's ``builders/synthetic/ns_2d.py`` on the CPU (by file: the package ``__init__`` files above it import h5py /
Lightning / jax) and writes tests/golden/ns2d_varying_ref.npz: on the initial vorticity, viscosities, grid (N = 16, B = 3), steps
(10 of 1e-2, two snapshots), cycles = 2, scaling = 0.1 and numpy seed of tests/golden/ns2d_ref.npz, the reference's fp32 ``sol``
and ``fs`` of ``varying_force=True`` for the random force with t_scaling = 20 and 0.2, each with a scalar and a per-sample
viscosity, and one run with ``force=li``, which the reference solves with the random force as well.  At t_scaling = 20 the phase
moves 0.2 rad a step, so a force that is frozen, a step late, or recorded at the snapshot's time is far outside the tests' bounds;
at the default 0.2 a one-step slip is about 1e-5.  Also the amplitudes [cycles, 6, B] of the force, drawn here with a CPU
generator on the seed the solver draws from numpy.  Only data is written; nothing of the reference's text.

Usage:  python tools/make_golden_ns2d_varying.py /path/to/reference      (or FFNO_REFERENCE=/path/to/reference)
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
    sys.exit("usage: python tools/make_golden_ns2d_varying.py /path/to/reference   (or FFNO_REFERENCE=...)")
BASE = os.path.join(ROOT, "tests", "golden", "ns2d_ref.npz")
OUT = os.path.join(ROOT, "tests", "golden", "ns2d_varying_ref.npz")
T_SCALINGS = (20.0, 0.2)


def load(name):
    spec = importlib.util.spec_from_file_location(f"reference_{name}", os.path.join(SYN, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ns = load("ns_2d")
    base = dict(np.load(BASE))
    B, N, STEPS, RECORDS, CYCLES, NUMPY_SEED, _ = (int(v) for v in base["shape"])
    DT, SCALING = float(base["dt"]), float(base["scaling"])
    w0 = torch.from_numpy(base["w0"])
    visc = {"scalar": float(base["visc_scalar"]), "array": base["visc_array"]}

    np.random.seed(NUMPY_SEED)
    gen = torch.Generator("cpu")
    gen.manual_seed(int(np.random.randint(1, 1000000000)))
    amplitudes = torch.stack([torch.rand(B, 1, 1, generator=gen).reshape(B) for _ in range(6 * CYCLES)]).reshape(CYCLES, 6, B)

    arrays = dict(shape=base["shape"], dt=base["dt"], scaling=base["scaling"], t_scalings=np.array(T_SCALINGS), w0=base["w0"],
                  visc_array=base["visc_array"], visc_scalar=base["visc_scalar"], amplitudes=amplitudes.numpy())

    def run(force, vname, t_scaling):
        np.random.seed(NUMPY_SEED)
        sol, fs = ns.solve_navier_stokes_2d(w0.clone(), visc[vname], STEPS * DT, DT, RECORDS, CYCLES, SCALING, t_scaling,
                                            ns.Force(force), True)
        assert sol.shape == fs.shape == (B, N, N, RECORDS)
        return sol.astype(np.float32), np.asarray(fs, np.float32)

    for t_scaling in T_SCALINGS:
        for vname in visc:
            sol, fs = run("random", vname, t_scaling)
            arrays[f"random.{t_scaling:g}.{vname}.sol"] = sol
            if vname == "scalar":      # (the force does not depend on the viscosity)
                arrays[f"random.{t_scaling:g}.fs"] = fs
    arrays["li.20.scalar.sol"], arrays["li.20.fs"] = run("li", "scalar", 20.0)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
