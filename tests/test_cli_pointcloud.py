"""`python -m fourierflow_amd {train,test,predict}` for the point-cloud routine: a `--data` file with the arrays `xy`, `rr`,
`sigma`, two optimisation steps, the checkpoint layout of the other routines; synthetic point clouds take `--size`."""
import json
import os

import numpy as np
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401

POINTCLOUD = """
routine:
  _target_: fourierflow.routines.PointCloudExperiment
  model:
    _target_: fourierflow.modules.FNOFactorizedPointCloud2D
    modes1: 4
    modes2: 3
    s1: 10
    s2: 12
    width: 32
    in_channels: 2
    out_channels: 1
    n_layers: 2
  iphi:
    _target_: fourierflow.modules.IPhi
    width: 16
  N: 10
  optimizer:
    _target_: functools.partial
    _args_: ["${get_method: torch.optim.AdamW}"]
    lr: 0.001
    weight_decay: 0.0001
  scheduler:
    scheduler:
      _target_: functools.partial
      _args_: ["${get_method: fourierflow.schedulers.CosineWithWarmupScheduler}"]
      num_warmup_steps: 2
      num_training_steps: 100
      num_cycles: 0.5
builder:
  batch_size: 2
"""


def _run(args, device):
    from fourierflow_amd.cli import app
    res = CliRunner().invoke(app, [*args, "--device", device])
    assert res.exit_code == 0, (res.output, res.exception)
    return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]


def test_cli_pointcloud_train_test_predict(tmp_path, host_device):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(POINTCLOUD)
    rng = np.random.default_rng(0)
    data = tmp_path / "data.npz"
    np.savez(data, xy=rng.uniform(0, 1, (4, 37, 2)).astype(np.float32), rr=rng.standard_normal((4, 42)).astype(np.float32),
             sigma=rng.standard_normal((4, 37, 1)).astype(np.float32))
    out = _run(["train", str(cfg), "--steps", "2", "--data", str(data), "--checkpoint-id", "pc"], host_device)
    assert [o["step"] for o in out[:-1]] == [0, 1]
    assert abs(out[0]["lr"] - 0.0005) < 1e-12 and abs(out[1]["lr"] - 0.001) < 1e-12      # the lr of the NEXT step: warm-up over 2
    assert all(np.isfinite(o["train_loss"]) for o in out[:-1]) and np.isfinite(out[-1]["valid_loss"])
    files = sorted(os.listdir(tmp_path / "checkpoints" / "trial-0-pc"))
    assert files[1] == "last.ckpt" and files[0].startswith("epoch=0-step=2-valid_loss=")
    t = _run(["test", str(cfg), "--data", str(data)], host_device)[-1]
    assert t["checkpoint"].endswith(files[0]) and np.isfinite(t["test_loss"])
    p = _run(["predict", str(cfg), "--size", "50", "--batch-size", "2"], host_device)[-1]      # synthetic points
    assert p["shape"] == [2, 50, 1] and np.isfinite(np.load(p["predictions"])["preds"]).all()
    bad = tmp_path / "bad.npz"
    np.savez(bad, x=np.zeros((2, 4, 2), np.float32))
    from fourierflow_amd.cli import app
    res = CliRunner().invoke(app, ["train", str(cfg), "--data", str(bad), "--device", host_device])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError)
