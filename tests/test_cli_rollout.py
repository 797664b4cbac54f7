"""`python -m fourierflow_amd rollout CONFIG.yaml --init IC.npz`: the trained Markov routine as a simulator (the reference's
`fourierflow infer`, commands/infer.py) -- initial conditions in, trajectories and the time per step out."""
import json
import os

import numpy as np
import pytest
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
    input_dim: {input_dim}
    share_weight: true
    factor: 4
    ff_weight_norm: true
    gain: 0.1
  n_steps: 3
  step_size: 0.5
  max_accumulations: 100
  noise_std: 0.0
  append_force: {force}
  append_mu: {force}
builder:
  batch_size: 2
"""
ROLLOUT_CONFIG = """
routine:
  _target_: fourierflow.routines.Grid2DRolloutExperiment
  conv:
    _target_: fourierflow.modules.FNOFactorized2DBlock
    modes: 4
    width: 32
    n_layers: 2
    input_dim: 12
    share_weight: true
    factor: 4
    ff_weight_norm: true
    gain: 0.1
  n_steps: 2
"""
G, N, STEPS = 8, 3, 4
KEYS = {"checkpoint", "predictions", "shape", "ms_per_step", "finite", "inference_time"}


def _invoke(args, device):
    from fourierflow_amd.cli import app
    return CliRunner().invoke(app, [*args, "--device", device])


def _run(args, device):
    res = _invoke(args, device)
    assert res.exit_code == 0, (res.output, res.exception)
    return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]


def _trained(tmp_path, device, force=False):
    cfg = tmp_path / "config.yaml"
    cfg.write_text(CONFIG.format(input_dim=5 if force else 3, force="true" if force else "false"))
    _run(["train", str(cfg), "--steps", "2", "--grid", str(G), "--accumulation-batches", "1"], device)
    from fourierflow_amd.cli import _last_routine
    return cfg, _last_routine()


def _simulate(routine, device, x0, steps, f=None, mu=None, every=1):
    was_training = routine.training
    routine.eval()
    dev = lambda a: None if a is None else torch.from_numpy(a).to(device)      # noqa: E731
    out = routine.simulate(dev(x0), steps, dev(f), dev(mu), every=every).cpu().numpy()
    routine.train(was_training)
    return out


def test_cli_rollout_round_trip_and_chunks(tmp_path, host_device):
    cfg, routine = _trained(tmp_path, host_device)
    rs = np.random.RandomState(3)
    x0 = rs.standard_normal((N, G, G)).astype(np.float32)
    ic = tmp_path / "ic.npz"
    np.savez(ic, x0=x0)
    out = _run(["rollout", str(cfg), "--init", str(ic), "--steps", str(STEPS), "--every", "2"], host_device)[-1]
    assert KEYS <= set(out), sorted(out)
    tdir = tmp_path / "checkpoints" / os.listdir(tmp_path / "checkpoints")[0]
    assert out["checkpoint"].startswith(str(tdir / "epoch")) and out["predictions"] == str(tdir / "rollout.npz")
    assert out["shape"] == [N, G, G, STEPS // 2] and out["finite"] is True and out["ms_per_step"] > 0
    assert out["inference_time"] == pytest.approx(out["elapsed"] / N / (0.5 * STEPS))
    with np.load(out["predictions"]) as z:
        preds, times = z["preds"], z["times"]
    want = _simulate(routine, host_device, x0, STEPS, every=2)
    assert np.array_equal(preds, want)
    assert np.array_equal(times, np.array([1.0, 2.0], np.float32))             # step_size 0.5 * every 2 * (1, 2)
    # a chunk boundary: 2 + 1 samples give what the 3 give at once, bit for bit (the samples of a batch do not see each other)
    other = tmp_path / "chunks.npz"
    two = _run(["rollout", str(cfg), "--init", str(ic), "--steps", str(STEPS), "--every", "2", "--batch-size", "2", "--output",
                str(other)], host_device)[-1]
    assert two["predictions"] == str(other) and two["shape"] == out["shape"]
    with np.load(other) as z:
        chunks = z["preds"]
    assert np.array_equal(chunks[:2], _simulate(routine, host_device, x0[:2], STEPS, every=2))
    assert np.array_equal(chunks[2:], _simulate(routine, host_device, x0[2:], STEPS, every=2))
    print("chunks vs one chunk: max abs diff", float(np.abs(chunks - preds).max()), "rel l2", float(np.linalg.norm(chunks - preds) / np.linalg.norm(preds)))
    assert np.array_equal(chunks, preds)


def test_cli_rollout_takes_force_and_viscosity_and_a_trajectory_array(tmp_path, host_device):
    cfg, routine = _trained(tmp_path, host_device, force=True)
    rs = np.random.RandomState(4)
    data = rs.standard_normal((N, G, G, 5)).astype(np.float32)
    f = rs.standard_normal((N, G, G, STEPS + 1)).astype(np.float32)
    mu = rs.uniform(0.1, 1.0, N).astype(np.float32)
    ic = tmp_path / "ic.npz"
    np.savez(ic, data=data, f=f, mu=mu)
    out = _run(["rollout", str(cfg), "--init", str(ic), "--steps", str(STEPS)], host_device)[-1]
    with np.load(out["predictions"]) as z:
        preds, times = z["preds"], z["times"]
    assert np.array_equal(preds, _simulate(routine, host_device, data[..., 0], STEPS, f, mu))
    assert np.array_equal(times, 0.5 * np.arange(1, STEPS + 1, dtype=np.float32))


def test_cli_rollout_refusals(tmp_path, host_device):
    cfg, _ = _trained(tmp_path, host_device, force=True)
    rs = np.random.RandomState(5)
    x0 = rs.standard_normal((N, G, G)).astype(np.float32)
    nothing, no_f, no_mu, flat = (tmp_path / f"{k}.npz" for k in ("nothing", "no_f", "no_mu", "flat"))
    np.savez(nothing, x=x0[..., None], y=x0[..., None])
    np.savez(no_f, x0=x0, mu=np.ones(N, np.float32))
    np.savez(no_mu, vorticity=x0, f=x0)
    np.savez(flat, x0=x0[0], f=x0, mu=np.ones(N, np.float32))
    other = tmp_path / "other"
    other.mkdir()
    rcfg = other / "config.yaml"
    rcfg.write_text(ROLLOUT_CONFIG)
    for args, word in ((["rollout", str(cfg), "--init", str(nothing)], "none of the arrays x0, vorticity, data"),
                       (["rollout", str(cfg), "--init", str(no_f)], "['f'] missing"),
                       (["rollout", str(cfg), "--init", str(no_mu)], "['mu'] missing"),
                       (["rollout", str(cfg), "--init", str(flat)], "must be [n, M, N]"),
                       (["rollout", str(cfg), "--init", str(no_f), "--steps", "5", "--every", "2"], "multiple of --every"),
                       (["rollout", str(rcfg), "--init", str(no_f)], "runs the Markov routine")):
        res = _invoke(args, host_device)
        assert res.exit_code != 0 and isinstance(res.exception, ValueError) and word in str(res.exception), (args, res.exception)
    assert _invoke(["rollout", str(cfg)], host_device).exit_code != 0          # --init is required
