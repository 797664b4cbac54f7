"""`python -m fourierflow_amd train CONFIG <override> --builder --epochs E` / `test CONFIG <override> --builder` on a geo-FNO
elasticity config (PointCloudExperiment + fourierflow.modules.FNOPointCloud2D + IPhi, torch.optim.Adam + StepLR, ElasticityBuilder)
over tiny synthetic .npy files: the best checkpoint and last.ckpt are written, StepLR falls per epoch, `test` reports the
checkpoint's test loss."""
import json
import os

import numpy as np
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401

OVERRIDE = "routine.model._target_=fourierflow_amd.modules.FNOPointCloud2D"
N_FILE, TRAIN, VALID, TEST, B, P = 10, 4, 2, 2, 2, 37

GEOFNO = """
routine:
  _target_: fourierflow.routines.PointCloudExperiment
  model:
    _target_: fourierflow.modules.FNOPointCloud2D
    modes1: 3
    modes2: 2
    s1: 8
    s2: 10
    width: 32
    in_channels: 2
    out_channels: 1
    n_layers: 3
  iphi:
    _target_: fourierflow.modules.IPhi
    width: 16
  N: 10
  optimizer:
    _target_: functools.partial
    _args_: ["${get_method: torch.optim.Adam}"]
    lr: 0.001
    weight_decay: 0.0001
  scheduler:
    scheduler:
      _target_: functools.partial
      _args_: ["${get_method: torch.optim.lr_scheduler.StepLR}"]
      step_size: 1
      gamma: 0.5
    name: learning_rate
    interval: epoch
    frequency: 1
    monitor: null
builder:
  _target_: fourierflow.builders.ElasticityBuilder
  sigma_path: ${oc.env:DATA_ROOT}/sigma.npy
  xy_path: ${oc.env:DATA_ROOT}/xy.npy
  rr_path: ${oc.env:DATA_ROOT}/rr.npy
  train_size: %d
  valid_size: %d
  test_size: %d
  batch_size: %d
  num_workers: 1
trainer:
  max_epochs: 501
""" % (TRAIN, VALID, TEST, B)


def _invoke(args, device):
    from fourierflow_amd.cli import app
    return CliRunner().invoke(app, [*args, "--device", device])


def _lines(res):
    assert res.exit_code == 0, (res.output, res.exception)
    return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]


def test_geofno_config_trains_and_tests_from_the_elasticity_files(tmp_path, host_device, monkeypatch):
    rs = np.random.RandomState(73)
    for name, a in (("rr", rs.standard_normal((42, N_FILE))), ("sigma", rs.standard_normal((P, N_FILE))),
                    ("xy", rs.uniform(0, 1, (P, 2, N_FILE)))):
        np.save(tmp_path / f"{name}.npy", a)
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(GEOFNO)

    res = _invoke(["train", str(cfg), "--builder", "--no-logging"], host_device)       # without the override: today's message
    assert res.exit_code != 0 and isinstance(res.exception, NotImplementedError) and "FNOPointCloud2D" in str(res.exception)

    out = _lines(_invoke(["train", str(cfg), OVERRIDE, "--builder", "--epochs", "2", "--checkpoint-id", "g"], host_device))
    log, summary = out[:-1], out[-1]
    from fourierflow_amd.cli import _last_routine
    routine = _last_routine()
    assert type(routine.model).__name__ == "FNOPointCloud2D" and routine.optimizer_type == "adam"
    assert [l["epoch"] for l in log] == [1, 2] and [l["step"] for l in log] == [2, 4]
    assert [l["lr"] for l in log] == [1e-3, 5e-4]                       # StepLR(1, 0.5): the lr each epoch ran with
    assert routine.current_epoch == 2 and routine.trainer().current_lr() == 2.5e-4
    assert all(np.isfinite(l["train_loss"]) and np.isfinite(l["valid_loss"]) for l in log)
    assert summary["steps"] == 4 and summary["epochs"] == 2
    files = sorted(os.listdir(tmp_path / "checkpoints" / "trial-0-g"))
    assert len(files) == 2 and files[1] == "last.ckpt" and files[0].startswith("epoch=")
    best = min(log, key=lambda l: l["valid_loss"])
    assert files[0].startswith(f"epoch={best['epoch']}-step={best['step']}-valid_loss=")

    t = _lines(_invoke(["test", str(cfg), OVERRIDE, "--builder"], host_device))[-1]
    assert t["checkpoint"].endswith(files[0]) and np.isfinite(t["test_loss"])
    # the test loss is the checkpoint's: the routine rebuilt from the file gives it on the builder's test split
    import torch
    from fourierflow_amd.builders import ElasticityBuilder
    from fourierflow_amd.config import build_routine, load_config
    fresh = build_routine(load_config(str(cfg), [OVERRIDE]))
    fresh.load_lightning_model_state(str(tmp_path / "checkpoints" / "trial-0-g" / files[0]))
    fresh.to(host_device)
    bld = ElasticityBuilder(str(tmp_path / "sigma.npy"), str(tmp_path / "xy.npy"), str(tmp_path / "rr.npy"), TRAIN, VALID, TEST,
                            batch_size=B)
    batch = next(iter(bld.test_data(torch.device(host_device)).epoch()))
    assert abs(float(fresh.test_step(batch)) - t["test_loss"]) <= 1e-6 * max(1.0, abs(t["test_loss"]))
