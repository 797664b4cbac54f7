"""`train --valid-data TRAJ.npz` and `test --data TRAJ.npz` for the Markov routine: a file with `data` [n, M, N, T] is a
trajectory file, validated / tested with the autoregressive metrics of validation_step / test_step (reference
routines/grid_2d_markov.py:392-416) instead of the one-step loss of an (x, y) pair."""
import json
import os

import numpy as np
import torch
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401

CONFIG = """
routine:
  _target_: fourierflow.routines.Grid2DMarkovExperiment
  conv:
    _target_: fourierflow.modules.FNOFactorized2DBlock
    modes: 4
    width: 32
    n_layers: 2
    input_dim: 3
    share_weight: true
    factor: 4
    ff_weight_norm: true
    gain: 0.1
  n_steps: 3
  step_size: 0.5
  max_accumulations: 100
  noise_std: 0.0
builder:
  batch_size: 2
"""
G, T = 8, 6


def _invoke(args, device):
    from fourierflow_amd.cli import app
    return CliRunner().invoke(app, [*args, "--device", device])


def _run(args, device):
    res = _invoke(args, device)
    assert res.exit_code == 0, (res.output, res.exception)
    return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]


def test_cli_validates_and_tests_on_a_trajectory_file(tmp_path, host_device):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG)
    rs = np.random.RandomState(0)
    data = rs.standard_normal((4, G, G, T)).astype(np.float32)
    times = np.tile(np.arange(T, dtype=np.float32) * 0.5, (4, 1))
    traj = tmp_path / "traj.npz"
    np.savez(traj, data=data, times=times, corr_data=data)
    out = _run(["train", str(cfg), "--steps", "2", "--grid", str(G), "--accumulation-batches", "1", "--valid-data", str(traj)],
               host_device)[-1]
    tdir = tmp_path / "checkpoints" / os.listdir(tmp_path / "checkpoints")[0]
    best = [f for f in os.listdir(tdir) if f.startswith("epoch")]
    assert len(best) == 1 and out["checkpoint"].endswith(best[0])
    # the file name carries the TRAJECTORY valid_loss: validation_step of the trained routine on the first batch of the file
    from fourierflow_amd.cli import _last_routine
    routine = _last_routine()
    was_training = routine.training
    routine.eval()
    v = routine.validation_step({k: torch.from_numpy(a[:2]).to(host_device) for k, a in
                                 dict(data=data, times=times, corr_data=data).items()})
    routine.train(was_training)
    assert best[0] == f"epoch=1-step=2-valid_loss={float(v['valid_loss']):.5f}.ckpt"
    assert out["valid_loss"] == round(float(v["valid_loss"]), 6)
    t = _run(["test", str(cfg), "--data", str(traj), "--batches", "2"], host_device)[-1]
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr"}
    assert t["checkpoint"].endswith(best[0]) and t["test_loss"] > 0 and t["test_loss_avg"] > 0
    assert 0.0 <= t["test_time_until"] <= 3 * 0.5 and -1.0 <= t["test_corr"] <= 1.0
    # the first of the two averaged batches is the validation batch
    routine.eval()
    second = routine.test_step({"data": torch.from_numpy(data[2:]).to(host_device)})
    assert abs(t["test_loss"] - (float(v["valid_loss"]) + float(second["test_loss"])) / 2) < 2e-6


def test_cli_refuses_misplaced_trajectory_files(tmp_path, host_device):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG)
    rs = np.random.RandomState(1)
    traj, pairs, short = tmp_path / "traj.npz", tmp_path / "pairs.npz", tmp_path / "short.npz"
    np.savez(traj, data=rs.standard_normal((2, G, G, T)).astype(np.float32))
    np.savez(pairs, x=rs.standard_normal((2, G, G, 1)).astype(np.float32), y=rs.standard_normal((2, G, G, 1)).astype(np.float32))
    np.savez(short, data=rs.standard_normal((1, G, G, T)).astype(np.float32))
    for args, word in ((["train", str(cfg), "--steps", "1", "--no-logging", "--data", str(traj)], "--valid-data"),
                       (["train", str(cfg), "--steps", "1", "--no-logging", "--valid-data", str(pairs)], "no `data`"),
                       (["train", str(cfg), "--steps", "1", "--no-logging", "--valid-data", str(short)], "do not fill")):
        res = _invoke(args, host_device)
        assert res.exit_code != 0 and isinstance(res.exception, ValueError) and word in str(res.exception), (args, res.exception)
