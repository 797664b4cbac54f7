"""`python -m fourierflow_amd {train,test,predict}` with a config that names fourierflow.modules.FNOFullyFactorizedMesh2D: two
optimisation steps on a `--data` file, the checkpoint layout of the other routines, the checkpoint's test loss, synthetic point
clouds with `--size`; `train --builder` on tiny elasticity .npy files; and examples/elasticity_fully_factorized.yaml builds."""
import json
import os

import numpy as np
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN, VALID, TEST, P, N_FILE = 4, 2, 2, 37, 10

CONFIG = """
routine:
  _target_: fourierflow.routines.PointCloudExperiment
  model:
    _target_: fourierflow.modules.FNOFullyFactorizedMesh2D
    modes1: 4
    modes2: 3
    s1: 10
    s2: 10
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
  _target_: fourierflow.builders.ElasticityBuilder
  sigma_path: ${oc.env:DATA_ROOT}/sigma.npy
  xy_path: ${oc.env:DATA_ROOT}/xy.npy
  rr_path: ${oc.env:DATA_ROOT}/rr.npy
  train_size: %d
  valid_size: %d
  test_size: %d
  batch_size: 2
  num_workers: 1
""" % (TRAIN, VALID, TEST)


def _run(args, device):
    from fourierflow_amd.cli import app
    res = CliRunner().invoke(app, [*args, "--device", device])
    assert res.exit_code == 0, (res.output, res.exception)
    return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]


def test_cli_train_test_predict(tmp_path, host_device, monkeypatch):
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG)
    rng = np.random.default_rng(0)
    data = tmp_path / "data.npz"
    np.savez(data, xy=rng.uniform(0, 1, (4, P, 2)).astype(np.float32), rr=rng.standard_normal((4, 42)).astype(np.float32),
             sigma=rng.standard_normal((4, P, 1)).astype(np.float32))
    out = _run(["train", str(cfg), "--steps", "2", "--data", str(data), "--checkpoint-id", "ff"], host_device)
    from fourierflow_amd.cli import _last_routine
    routine = _last_routine()
    assert type(routine.model).__name__ == "FNOFullyFactorizedMesh2D" and routine.optimizer_type == "adamw"
    assert [o["step"] for o in out[:-1]] == [0, 1]
    assert abs(out[0]["lr"] - 0.0005) < 1e-12 and abs(out[1]["lr"] - 0.001) < 1e-12      # the lr of the NEXT step: warm-up over 2
    assert all(np.isfinite(o["train_loss"]) for o in out[:-1]) and np.isfinite(out[-1]["valid_loss"])
    files = sorted(os.listdir(tmp_path / "checkpoints" / "trial-0-ff"))
    assert files[1] == "last.ckpt" and files[0].startswith("epoch=0-step=2-valid_loss=")
    t = _run(["test", str(cfg), "--data", str(data)], host_device)[-1]
    assert t["checkpoint"].endswith(files[0]) and np.isfinite(t["test_loss"])
    p = _run(["predict", str(cfg), "--size", "50", "--batch-size", "2"], host_device)[-1]      # synthetic points
    assert p["shape"] == [2, 50, 1] and np.isfinite(np.load(p["predictions"])["preds"]).all()


def test_cli_trains_and_tests_from_the_elasticity_files(tmp_path, host_device, monkeypatch):
    rs = np.random.RandomState(74)
    for name, a in (("rr", rs.standard_normal((42, N_FILE))), ("sigma", rs.standard_normal((P, N_FILE))),
                    ("xy", rs.uniform(0, 1, (P, 2, N_FILE)))):
        np.save(tmp_path / f"{name}.npy", a)
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG)
    out = _run(["train", str(cfg), "--builder", "--epochs", "1", "--checkpoint-id", "b"], host_device)
    log, summary = out[:-1], out[-1]
    assert [l["epoch"] for l in log] == [1] and [l["step"] for l in log] == [2]
    assert all(np.isfinite(l["train_loss"]) and np.isfinite(l["valid_loss"]) for l in log)
    assert summary["steps"] == 2 and summary["epochs"] == 1
    files = sorted(os.listdir(tmp_path / "checkpoints" / "trial-0-b"))
    assert len(files) == 2 and files[1] == "last.ckpt" and files[0].startswith("epoch=1-step=2-valid_loss=")
    t = _run(["test", str(cfg), "--builder"], host_device)[-1]
    assert t["checkpoint"].endswith(files[0]) and np.isfinite(t["test_loss"])


def test_example_config_builds(monkeypatch):
    import yaml
    from fourierflow_amd.config import build_routine, load_config
    from fourierflow_amd.modules import FNOFullyFactorizedMesh2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    monkeypatch.setenv("DATA_ROOT", "/nowhere")
    path = os.path.join(ROOT, "examples", "elasticity_fully_factorized.yaml")
    routine = build_routine(load_config(path))
    raw = yaml.safe_load(open(path).read())["routine"]
    assert raw["model"]["_target_"] == "fourierflow.modules.FNOFullyFactorizedMesh2D"
    assert type(routine) is PointCloudExperiment and routine.N == raw["N"] and routine.optimizer_type == "adamw"
    assert type(routine.model) is FNOFullyFactorizedMesh2D and type(routine.iphi) is IPhi
    for k, v in raw["model"].items():
        if not k.startswith("_"):
            assert getattr(routine.model, k) == v, k
    assert routine.iphi.width == raw["iphi"]["width"]
    assert len(routine.model.convs) == raw["model"]["n_layers"] + 1 and len(routine.model.ws) == raw["model"]["n_layers"] - 1
    assert routine._opt_kw["lr"] == 0.001 and routine._opt_kw["weight_decay"] == 0.0001
    assert routine._sch_kw == dict(num_warmup_steps=500, num_training_steps=10000, num_cycles=0.5)
