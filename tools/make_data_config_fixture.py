"""Writes tests/golden/reference_data_configs.npz: the reference's data/kolmogorov/**/*.yaml files (the settings of `generate
kolmogorov`) as test data for tests/test_kf2d_data_configs.py and tests/test_cli_generate_kolmogorov.py (`paths`: path relative to
data/kolmogorov/, `texts`: the file's YAML text, both unicode arrays).

Usage:  python tools/make_data_config_fixture.py REFERENCE_CHECKOUT
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_data_configs.npz")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    top = os.path.join(sys.argv[1], "data", "kolmogorov")
    paths = sorted(os.path.relpath(p, top) for p in glob.glob(os.path.join(top, "**", "*.yaml"), recursive=True))
    if not paths:
        raise SystemExit(f"no data/kolmogorov/**/*.yaml under {sys.argv[1]}")
    texts = []
    for p in paths:
        with open(os.path.join(top, p)) as f:
            texts.append(f.read())
    np.savez_compressed(OUT, paths=np.array(paths), texts=np.array(texts))
    z = np.load(OUT)
    assert z["paths"].tolist() == paths and z["texts"].tolist() == texts
    print(f"{OUT}: {len(paths)} configs, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
