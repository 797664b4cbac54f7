"""`train | test | predict CONFIG --builder` for the torus_li routines: Grid2DMarkovExperiment on NSMarkovBuilder and
Grid2DRolloutExperiment on NSZongyiBuilder (builders/ns_data.py) -- the statistics epoch of the Markov routine, whole epochs
against loops written here, validation over the whole split averaged by batch size, the best checkpoint, resume, the refusals,
and the two shipped configs torus_li/markov/24_layers and torus_li/zongyi/4_layers.  Files of 7 trajectories the tests write
themselves; the smallest models the engines take.  Emulator and GPU."""
import json
import os

import numpy as np
import pytest
import scipy.io
import torch
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401
from test_builders_ns import _zongyi_want
from test_config import shipped_configs

N, G, T, TRAIN, TEST, B = 7, 16, 6, 4, 2, 3             # Markov: 16 pairs, six batches (3 3 3 3 3 1); rollout: 4 samples (3 1)
PAIRS, STEPS_PER_EPOCH = TRAIN * (T - 2), 6
SEED = 7231                                            # trial 0 of the CLI

MARKOV = """
routine:
  _target_: fourierflow.routines.Grid2DMarkovExperiment
  conv:
    _target_: fourierflow.modules.FNOFactorized2DBlock
    modes: 4
    width: 32
    n_layers: 1
    input_dim: 3
    share_weight: true
    factor: 4
    ff_weight_norm: true
    gain: 0.1
  n_steps: 3
  max_accumulations: 100
  noise_std: 0.0
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
  _target_: fourierflow.builders.NSMarkovBuilder
  data_path: ${oc.env:DATA_ROOT}/u.mat
  train_size: %d
  test_size: %d
  ssr: 1
  batch_size: %d
  num_workers: 4
  pin_memory: true
trainer:
  max_epochs: 3
""" % (TRAIN, TEST, B)
ROLLOUT = """
routine:
  _target_: fourierflow.routines.Grid2DRolloutExperiment
  conv:
    _target_: fourierflow.modules.FNOZongyi2DBlock
    modes1: 4
    modes2: 4
    width: 20
    n_layers: 1
    input_dim: 4
  n_steps: 2
  optimizer:
    _target_: functools.partial
    _args_: ["${get_method: torch.optim.AdamW}"]
    lr: 0.0025
    weight_decay: 0.0001
  scheduler:
    scheduler:
      _target_: functools.partial
      _args_: ["${get_method: torch.optim.lr_scheduler.StepLR}"]
      step_size: 1
      gamma: 0.5
builder:
  _target_: fourierflow.builders.NSZongyiBuilder
  data_path: ${oc.env:DATA_ROOT}/u.mat
  train_size: %d
  test_size: %d
  ssr: 1
  n_steps: 2
  batch_size: %d
  num_workers: 4
trainer:
  max_epochs: 2
""" % (TRAIN, TEST, B)

# the log line carries six decimals (half a unit of the sixth); the weighted mean of a few float32 values of order 1 accumulated
# in double against the same mean taken here differs by their float32 rounding at most
LOG_TOL = 0.5e-6 + 1e-6


def _invoke(args, device):
    from fourierflow_amd.cli import app
    return CliRunner().invoke(app, [*args, "--device", device])


def _run(args, device):
    """-> (log lines, summary line, the trained routine's state, its AdamW moments)"""
    res = _invoke(args, device)
    assert res.exit_code == 0, (res.output, res.exception)
    lines = [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]
    if args[0] != "train":
        return lines[:-1], lines[-1], None, None
    from fourierflow_amd.cli import _last_routine
    routine = _last_routine()
    state = {k: v.detach().cpu().numpy().copy() for k, v in routine.state_dict().items()}
    tr = routine.trainer()
    return lines[:-1], lines[-1], state, (tr.m.cpu().numpy().copy(), tr.v.cpu().numpy().copy())


def _same_state(a, b):
    assert set(a) == set(b) and len(a) >= 10
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture()
def files(tmp_path, monkeypatch):
    u = (np.random.RandomState(91).standard_normal((N, G, G, T)) + 0.3).astype(np.float32)
    scipy.io.savemat(tmp_path / "u.mat", {"u": u})
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    (tmp_path / "markov.yaml").write_text(MARKOV)
    (tmp_path / "rollout.yaml").write_text(ROLLOUT)
    return str(tmp_path / "markov.yaml"), str(tmp_path / "rollout.yaml"), tmp_path, u


def _fresh(cfg_path, device, overrides=()):
    """The routine as `train` builds it: seeded with 7231 + trial before construction."""
    from fourierflow_amd.config import build_routine, load_config
    torch.manual_seed(SEED)
    return build_routine(load_config(cfg_path, list(overrides))).to(device)


def _state(routine):
    return {k: v.detach().cpu().numpy().copy() for k, v in routine.state_dict().items()}


def _trial_files(root, trial=0):
    d = root / "checkpoints"
    tdir = d / [n for n in os.listdir(d) if n.startswith(f"trial-{trial}-")][0]
    return tdir, sorted(os.listdir(tdir))


def _weighted(routine, batches, step="validation_step"):
    """{key: mean over `batches` weighted by batch size} of the routine's step under eval()."""
    routine.eval()
    total, n = {}, 0
    with torch.no_grad():
        for b in batches:
            size = len(next(iter(b.values())))
            for k, v in getattr(routine, step)(b).items():
                if not torch.is_tensor(v) or v.numel() == 1:
                    total[k] = total.get(k, 0.0) + float(v) * size
            n += size
    return {k: v / n for k, v in total.items()}


def _trajectory_batches(u, size, device):
    times = np.arange(0, 20, dtype=np.float32)[:u.shape[-1]]
    return [dict(data=torch.from_numpy(u[lo:lo + size].copy()).to(device),
                 times=torch.from_numpy(np.tile(times, (len(u[lo:lo + size]), 1))).to(device)) for lo in range(0, len(u), size)]


def _window_batches(u, size, device):
    want = _zongyi_want(u, True)
    return [{k: torch.from_numpy(v[lo:lo + size].copy()).to(device) for k, v in want.items()} for lo in range(0, len(u), size)]


MARKOV_VALID = ("valid_loss", "valid_loss_avg", "valid_time_until", "valid_reduced_time_until", "valid_corr")
ROLLOUT_VALID = ("valid_loss", "valid_loss_avg", "valid_time_until")


# -- Markov ----------------------------------------------------------------------------------------------------------------------
def test_markov_statistics_epoch_changes_nothing_but_the_normaliser(files, host_device):
    cfg, _, root, _ = files
    log, summary, state, (m, v) = _run(["train", cfg, "--builder", "--epochs", "1", "--no-shuffle", "--checkpoint-id", "s"], host_device)
    assert [(l["epoch"], l["step"], l["train_loss"]) for l in log] == [(1, 0, None)] and summary["steps"] == 0
    initial = _state(_fresh(cfg, host_device))
    changed = [k for k in state if state[k].tobytes() != initial[k].tobytes()]
    assert changed and all(k.startswith("normalizer.") for k in changed), changed
    assert not m.any() and not v.any()
    # every pair once, pooled over the grid as the Normalizer counts its rows (normalizer.py:28-34); one accumulation per batch
    assert state["normalizer.count"] == PAIRS * G * G and state["normalizer.n_accumulations"] == STEPS_PER_EPOCH
    tdir, names = _trial_files(root)
    assert len(names) == 2 and names[0].startswith("epoch=1-step=0-valid_loss=") and names[1] == "last.ckpt"
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["epoch"] == 1 and last["global_step"] == 0
    opt = last["optimizer_states"][0]
    assert opt["step"] == 0 and not opt["exp_avg"].any() and not opt["exp_avg_sq"].any()
    assert last["lr_schedulers"][0]["last_epoch"] == 0
    for k, val in last["state_dict"].items():
        assert val.numpy().tobytes() == state[k].tobytes(), k


def test_markov_epochs_equal_the_hand_written_loop(files, host_device):
    from fourierflow_amd.builders import MarkovTrajectoryData
    cfg, _, root, u = files
    log, summary, state, _ = _run(["train", cfg, "--builder", "--no-shuffle", "--checkpoint-id", "a"], host_device)   # max_epochs = 3
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, STEPS_PER_EPOCH), (3, 2 * STEPS_PER_EPOCH)]
    assert log[0]["train_loss"] is None and all(np.isfinite(l["train_loss"]) for l in log[1:])
    assert summary["steps"] == 2 * STEPS_PER_EPOCH and summary["batch"] == B and summary["epochs"] == 3
    # the cosine schedule counts optimisation steps: warm-up of 2, so the epoch that only accumulated left it at step 0
    from fourierflow_amd.trainer import cosine_warmup_factor
    assert [l["lr"] for l in log] == [1e-3 * cosine_warmup_factor(s, 2, 100, 0.5) for s in (0, STEPS_PER_EPOCH, 2 * STEPS_PER_EPOCH)]
    routine = _fresh(cfg, host_device)
    ds = MarkovTrajectoryData(u[:TRAIN], device=host_device, batch_size=B, mode="ns_markov", k=1, seed=SEED, shuffle=False)
    losses = []
    for epoch in range(3):                                  # the whole statistics epoch, then two optimising epochs
        for batch in ds.epoch():
            losses.append(routine.training_step(batch, epoch=epoch))
    assert losses[:STEPS_PER_EPOCH] == [None] * STEPS_PER_EPOCH
    _same_state(state, _state(routine))
    assert log[-1]["train_loss"] == round(float(losses[-1].item()), 6)
    # the best file is the epoch of least valid_loss
    vls = [l["valid_loss"] for l in log]
    best = int(np.argmin(vls))
    assert [l["best"] for l in log] == [all(x < y for y in vls[:e]) for e, x in enumerate(vls)]
    tdir, names = _trial_files(root)
    assert len(names) == 2 and names[0].startswith(f"epoch={best + 1}-step={best * STEPS_PER_EPOCH}-valid_loss=") and names[1] == "last.ckpt"
    assert abs(float(names[0].rpartition("valid_loss=")[2][:-len(".ckpt")]) - vls[best]) <= 0.5e-5 + 1e-6


@pytest.mark.parametrize("test_size,batch", [(2, 3), (2, 1), (3, 2)])     # one batch of 2; two of 1; 2 + 1, where the weights differ
def test_markov_validation_keys_are_weighted_means_over_the_split(files, host_device, test_size, batch):
    cfg, _, root, u = files
    over = [f"builder.test_size={test_size}", f"builder.batch_size={batch}"]
    log, _, state, _ = _run(["train", cfg, *over, "--builder", "--epochs", "2", "--checkpoint-id", "v"], host_device)
    assert all(set(MARKOV_VALID) <= set(l) for l in log)
    tdir, _ = _trial_files(root)
    routine = _fresh(cfg, host_device)
    routine.load_lightning_model_state(str(tdir / "last.ckpt"))
    routine.to(host_device)
    want = _weighted(routine, _trajectory_batches(u[-test_size:], batch, host_device))
    assert set(want) == set(MARKOV_VALID)
    for k in MARKOV_VALID:
        assert abs(log[-1][k] - want[k]) <= LOG_TOL, (k, log[-1][k], want[k])
    # ... and `test --builder` reports the same means of test_step over the same trajectories, from the best checkpoint
    _, t, _, _ = _run(["test", cfg, *over, "--builder"], host_device)
    best = [n for n in _trial_files(root)[1] if n.startswith("epoch")][0]
    routine.load_lightning_model_state(str(tdir / best))
    routine.to(host_device)
    want = _weighted(routine, _trajectory_batches(u[-test_size:], batch, host_device), "test_step")
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr", "samples"}
    assert t["samples"] == test_size and t["checkpoint"].endswith(best)
    for k in ("test_loss", "test_loss_avg", "test_time_until", "test_corr"):
        assert abs(t[k] - want[k]) <= LOG_TOL, (k, t[k], want[k])


def test_markov_resumed_run_equals_the_uninterrupted_one(files, host_device):
    cfg, _, root, _ = files
    log_full, _, state_full, moments_full = _run(["train", cfg, "--builder", "--no-logging"], host_device)          # 3 epochs, shuffled
    _run(["train", cfg, "--builder", "--epochs", "2", "--checkpoint-id", "r"], host_device)                         # statistics + one
    log_res, summary, state_res, moments_res = _run(["train", cfg, "--builder", "--resume"], host_device)
    assert [l["epoch"] for l in log_res] == [3] and summary["resumed_from_step"] == STEPS_PER_EPOCH       # no second statistics epoch
    assert {k: v for k, v in log_res[0].items() if k != "best"} == {k: v for k, v in log_full[2].items() if k != "best"}
    _same_state(state_full, state_res)
    for a, b in zip(moments_full, moments_res):
        assert a.tobytes() == b.tobytes()
    assert state_res["normalizer.n_accumulations"] == 3 * STEPS_PER_EPOCH


def test_markov_predict(files, host_device):
    cfg, _, root, u = files
    _run(["train", cfg, "--builder", "--epochs", "2", "--checkpoint-id", "p"], host_device)
    _, one, _, _ = _run(["predict", cfg, "--builder"], host_device)
    assert one["shape"] == [N, G, G, 3] and one["samples"] == N and one["n_steps"] == 3 and one["step_size"] == 1.0
    assert one["inference_time"] > 0 and one["inference_time_ms_per_step"] > 0
    assert one["inference_time"] == pytest.approx(one["elapsed"] / N / (one["step_size"] * one["n_steps"]), rel=1e-12)
    whole = np.load(one["predictions"])["preds"]
    _, chunked, _, _ = _run(["predict", cfg, "--builder", "--batch-size", "3", "--output", str(root / "chunks.npz")], host_device)
    parts = np.load(chunked["predictions"])["preds"]
    assert parts.shape == whole.shape and np.isfinite(whole).all()
    # the same three model steps on the same trajectories, 3 + 3 + 1 at a time: fp32 passes whose reductions do not span the batch
    np.testing.assert_allclose(parts, whole, rtol=1e-4, atol=1e-5)


# -- rollout ---------------------------------------------------------------------------------------------------------------------
def test_rollout_epochs_equal_the_hand_written_loop(files, host_device):
    _, cfg, root, u = files
    log, summary, state, _ = _run(["train", cfg, "--builder", "--no-shuffle", "--checkpoint-id", "z"], host_device)   # max_epochs = 2
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 2), (2, 4)] and summary["steps"] == 4
    assert [l["lr"] for l in log] == [2.5e-3, 1.25e-3]                      # StepLR(step_size 1, gamma 0.5) advanced once per epoch
    from fourierflow_amd.cli import _last_routine
    assert _last_routine().current_epoch == 2
    routine = _fresh(cfg, host_device)
    step, loss = 0, None
    for _ in range(2):
        for batch in _window_batches(u[:TRAIN], B, host_device):
            loss = routine.training_step(batch, step)[0]
            step += 1
        routine.on_train_epoch_end()
    _same_state(state, _state(routine))
    assert log[-1]["train_loss"] == round(float(loss.item()), 6)
    # validation over the whole split (a batch of 2 here), test and predict
    assert all(set(ROLLOUT_VALID) <= set(l) for l in log)
    want = _weighted(routine, _window_batches(u[-TEST:], B, host_device))
    for k in ROLLOUT_VALID:
        assert abs(log[-1][k] - want[k]) <= LOG_TOL, (k, log[-1][k], want[k])
    vls = [l["valid_loss"] for l in log]
    best = int(np.argmin(vls))
    tdir, names = _trial_files(root)
    assert names[0].startswith(f"epoch={best + 1}-step={2 * (best + 1)}-valid_loss=") and names[1] == "last.ckpt"


@pytest.mark.parametrize("batch", [1, 3])
def test_rollout_validation_test_and_predict(files, host_device, batch):
    _, cfg, root, u = files
    over = ["builder.test_size=3", f"builder.batch_size={batch}"]                  # batches of 1 1 1, or of 3
    log, _, _, _ = _run(["train", cfg, *over, "--builder", "--epochs", "1", "--checkpoint-id", "t"], host_device)
    tdir, names = _trial_files(root)
    routine = _fresh(cfg, host_device)
    routine.load_lightning_model_state(str(tdir / names[0]))
    routine.to(host_device)
    want = _weighted(routine, _window_batches(u[-3:], batch, host_device))
    for k in ROLLOUT_VALID:
        assert abs(log[-1][k] - want[k]) <= LOG_TOL, (k, log[-1][k], want[k])
    _, t, _, _ = _run(["test", cfg, *over, "--builder"], host_device)
    want = _weighted(routine, _window_batches(u[-3:], batch, host_device), "test_step")
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "samples"} and t["samples"] == 3
    for k in ("test_loss", "test_loss_avg", "test_time_until"):
        assert abs(t[k] - want[k]) <= LOG_TOL, (k, t[k], want[k])
    _, p, _, _ = _run(["predict", cfg, "--builder", *(["--batch-size", "3"] if batch == 3 else [])], host_device)
    assert p["shape"] == [N, G, G, 2] and p["samples"] == N and p["n_steps"] == 2
    assert p["inference_time"] > 0
    assert p["inference_time"] == pytest.approx(p["elapsed"] / N / (p["step_size"] * p["n_steps"]), rel=1e-12)
    # routine.forward over the file's trajectories: the first two fields in, the next two predicted
    with torch.no_grad():
        routine.eval()
        direct = routine.forward({"data": torch.from_numpy(u.copy()).to(host_device)})[2].cpu().numpy()
    np.testing.assert_allclose(np.load(p["predictions"])["preds"], direct, rtol=1e-4, atol=1e-5)


# -- refusals --------------------------------------------------------------------------------------------------------------------
FIVE = ("StructuredMesh2DBuilder", "PlasticityBuilder", "ElasticityBuilder", "NSMarkovBuilder", "NSZongyiBuilder")


def test_refusals(files, host_device):
    markov, rollout, root, _ = files

    def refused(args, *words):
        res = _invoke(args, host_device)
        assert res.exit_code != 0 and isinstance(res.exception, ValueError), (args, res.exception)
        for word in words:
            assert word in str(res.exception), (word, res.exception)

    # a section that lacks required arguments: they are named, and so are the five builders
    (root / "bare.yaml").write_text(MARKOV.split("builder:")[0] + "builder:\n  _target_: fourierflow.builders.NSMarkovBuilder\n  batch_size: 3\n")
    refused(["train", str(root / "bare.yaml"), "--builder", "--epochs", "1", "--no-logging"], "data_path", "train_size", "test_size",
            "ssr", *FIVE)
    refused(["train", rollout, "builder._target_=fourierflow.builders.NSMarkovBuilder", "--builder", "--no-logging"], "NSMarkovBuilder",
            *FIVE)                                                                            # the Markov builder under the rollout routine
    refused(["train", markov, "builder._target_=fourierflow.builders.NSZongyiBuilder", "--builder", "--no-logging"], "NSZongyiBuilder",
            *FIVE)                                                                            # ... and the reverse
    (root / "none.yaml").write_text(MARKOV.split("builder:")[0])
    refused(["train", str(root / "none.yaml"), "--builder", "--epochs", "1", "--no-logging"], "(none)", *FIVE)
    np.savez(root / "traj.npz", data=np.zeros((2, G, G, T), np.float32))
    for cmd in ("train", "test", "predict"):
        refused([cmd, markov, "--builder", "--data", str(root / "traj.npz")], "--data")
    # a builder whose windows do not fit the routine's rollout
    refused(["train", rollout, "builder.n_steps=3", "--builder", "--no-logging"], "n_steps = 3")


# -- the shipped configs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel,steps", [("torus_li/markov/24_layers", 0), ("torus_li/zongyi/4_layers", 1)])
def test_shipped_torus_li_configs_train_through_their_builder(tmp_path, monkeypatch, host_device, rel, steps):
    """The config files as shipped, on a file of 3 trajectories at the place and under the name they give (grid 32, which holds
    their 16 and 12 modes; T = 20): one layer, one epoch -- and the two split sizes, which the builders hold against the file.
    The Markov config's first epoch is its statistics epoch: it validates and writes its checkpoint at step 0."""
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()[rel + "/config.yaml"])
    os.makedirs(tmp_path / "zongyi")
    u = (np.random.RandomState(92).standard_normal((3, 32, 32, 20)) + 0.3).astype(np.float32)
    scipy.io.savemat(tmp_path / "zongyi" / "NavierStokes_V1e-5_N1200_T20.mat", {"u": u})
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    log, summary, _, _ = _run(["train", str(cfg), "routine.conv.n_layers=1", "builder.train_size=2", "builder.test_size=1", "--builder",
                               "--epochs", "1"], host_device)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, steps)] and np.isfinite(log[0]["valid_loss"]) and log[0]["best"]
    assert summary["batch"] == (19 if "markov" in rel else 20)
    tdir, names = _trial_files(tmp_path)
    assert len(names) == 2 and names[0].startswith(f"epoch=1-step={steps}-valid_loss=") and names[1] == "last.ckpt"
    assert torch.load(tdir / names[0], map_location="cpu", weights_only=False)["global_step"] == steps
