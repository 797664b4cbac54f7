#!/usr/bin/env python3
"""Golden data for NSContextualBuilder from the REAL reference datasets (build machine only; needs a reference checkout).

Loads the reference's ``builders/ns_contextual.py`` on the CPU and writes tests/golden/contextual_ref.npz: a tiny seeded set
(``u [3, 8, 8, 7]``, ``f`` once as ``[3, 8, 8]`` and once as ``[3, 8, 8, 7]``, ``mu [3]``; ssr = 2, k = 2) and, for both force
layouts, what ``NavierStokesTrainingDataset[idx]`` returns for every idx and what ``NavierStokesDataset[b]`` returns for every b,
``times`` included, stacked along a first axis.  Only data is written; nothing of the reference's text.

Two obstacles, both handled here without touching the checkout:
  * the reference's package ``__init__`` files import Lightning / hydra: synthetic parent packages (``__path__`` only) are
    registered first, so that just the one module file loads;
  * that module imports ``h5py`` (not installed, and not needed: the two dataset classes only index their ``data`` argument, so
    a dict of numpy arrays serves as the HDF5 group) and ``.base`` (a Lightning data module): both are empty stub modules.

Usage:  python tools/make_golden_contextual.py /path/to/reference      (or FFNO_REFERENCE=/path/to/reference)
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FFNO_REFERENCE")
if not REF or not os.path.isfile(os.path.join(REF, "fourierflow", "builders", "ns_contextual.py")):
    sys.exit("usage: python tools/make_golden_contextual.py /path/to/reference   (or FFNO_REFERENCE=...)")
OUT = os.path.join(ROOT, "tests", "golden", "contextual_ref.npz")

N, G, T, SSR, K = 3, 8, 7, 2, 2


def reference_datasets():
    for name, rel in (("fourierflow", "fourierflow"), ("fourierflow.builders", "fourierflow/builders")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    base = types.ModuleType("fourierflow.builders.base")
    base.Builder = type("Builder", (), {})
    sys.modules["fourierflow.builders.base"] = base
    mod = importlib.import_module("fourierflow.builders.ns_contextual")
    return mod.NavierStokesTrainingDataset, mod.NavierStokesDataset


def stack(items):
    return {key: np.stack([np.asarray(it[key]) for it in items]) for key in items[0]}


def main():
    Train, Eval = reference_datasets()
    rs = np.random.RandomState(20)
    u = (rs.standard_normal((N, G, G, T)) + 0.3).astype(np.float32)
    f_const = rs.standard_normal((N, G, G)).astype(np.float32)
    f_step = rs.standard_normal((N, G, G, T)).astype(np.float32)
    mu = rs.uniform(1e-5, 1e-3, N).astype(np.float32)
    arrays = dict(u=u, f_const=f_const, f_step=f_step, mu=mu, ssr=np.int64(SSR), k=np.int64(K))
    for tag, f in (("const", f_const), ("step", f_step)):
        group = dict(u=u, f=f, mu=mu)
        train, held = Train(group, SSR, K), Eval(group, SSR, K)
        assert len(train) == N * (T - K) and len(held) == N
        for split, ds in (("train", train), ("eval", held)):
            for key, value in stack([ds[i] for i in range(len(ds))]).items():
                arrays[f"{tag}.{split}.{key}"] = value
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB, {len(arrays)} arrays)")
    for name, a in arrays.items():
        print(f"  {name:20s} {a.dtype} {a.shape}")


if __name__ == "__main__":
    main()
