"""`python bench.py` without `--full`: the headline line only, `--steps` timed steps, and `--dump-outputs DIR` writing what the
last timed step left its caller (loss, flat parameters, AdamW moments) as float32 .npy files."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_output_dump(tmp_path):
    env = dict(os.environ)
    env.pop("RANK", None)
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["per_gpu_batch"] == 4
    assert d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-2 * d["ms_per_step"]
    assert "3 steps in" in r.stderr
    for k in ("roofline", "kernels", "cpu_baseline", "secondary", "ms_per_forward", "bf16_storage_variant"):
        assert k not in d, k                                  # measured only under --full
    n = int(re.search(r"all_reduce\(flat fp32 grads, (\d+) floats\)", d["config"]["collective"]).group(1))
    got = {name: np.load(out / f"{name}.npy") for name in ("loss", "params", "adam_m", "adam_v")}
    assert sorted(os.listdir(out)) == sorted(f"{name}.npy" for name in got)
    assert got["loss"].shape == (1,) and abs(float(got["loss"][0]) - d["final_loss"]) <= 1e-5
    for name in ("params", "adam_m", "adam_v"):
        a = got[name]
        assert a.dtype == np.float32 and a.shape == (n,) and np.isfinite(a).all(), name
    assert (got["adam_v"] >= 0).all() and np.abs(got["adam_m"]).max() > 0
