"""`train CONFIG --builder` / `test CONFIG --builder`: the mesh and point-cloud routines trained on the dataset files of the
config's `builder` section (builders/mesh_data.py) in whole epochs drawn on the device, validated on the held-out split after
every epoch, the best checkpoint kept.  Unshuffled, the run equals `train --data` on an .npz of the training split bit for bit.
Files of 12 samples the test writes itself; the smallest models the routine tests use.  Emulator and GPU."""
import json
import os

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401

X, Y, C = 6, 5, 3
N_FILE, TRAIN, VALID, TEST, B = 12, 4, 3, 3, 2           # 2 training batches per epoch; validation and test: 2 + 1
OUTPUT_DIM = 1

MESH_MODEL = """
  model:
    _target_: fourierflow.modules.FNOFactorizedMesh2D
    modes_x: 3
    modes_y: 2
    width: 32
    input_dim: 4
    n_layers: 2
    share_weight: false
    factor: 4
    ff_weight_norm: true
    n_ff_layers: 2
    layer_norm: false
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
"""
GEO_MODEL = """
  model:
    _target_: fourierflow.modules.FNOMesh2D
    modes1: 3
    modes2: 2
    width: 32
    n_layers: 3
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
"""
MESH_BUILDER = """
builder:
  _target_: fourierflow.builders.StructuredMesh2DBuilder
  x1_path: ${oc.env:DATA_ROOT}/X.npy
  x2_path: ${oc.env:DATA_ROOT}/Y.npy
  sigma_path: ${oc.env:DATA_ROOT}/Q.npy
  output_dim: %d
  train_size: %d
  valid_size: %d
  test_size: %d
  batch_size: %d
  num_workers: 1
  pin_memory: true
trainer:
  max_epochs: 3
""" % (OUTPUT_DIM, TRAIN, VALID, TEST, B)
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
  max_epochs: 2
""" % (TRAIN, VALID, TEST, B)


def _mesh_config(model=MESH_MODEL):
    return "routine:\n  _target_: fourierflow.routines.StructuredMeshExperiment" + model + MESH_BUILDER


def _invoke(args, device):
    from fourierflow_amd.cli import app
    return CliRunner().invoke(app, [*args, "--device", device])


def _run(args, device):
    """-> (log lines, summary line, the trained routine's state)"""
    res = _invoke(args, device)
    assert res.exit_code == 0, (res.output, res.exception)
    from fourierflow_amd.cli import _last_routine
    lines = [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]
    routine = _last_routine()
    state = {k: v.detach().cpu().numpy().copy() for k, v in routine.state_dict().items()} if args[0] == "train" else None
    return lines[:-1], lines[-1], state


@pytest.fixture()
def mesh(tmp_path, monkeypatch):
    """The three airfoil-style files and the same splits as .npz files of the npz path (structured_mesh_2d.py:40-46: train [:i],
    test [i:j], valid [j:k])."""
    rs = np.random.RandomState(71)
    x1, x2 = rs.standard_normal((N_FILE, X, Y)), rs.standard_normal((N_FILE, X, Y))
    q = rs.standard_normal((N_FILE, C, X, Y))
    for name, a in (("X", x1), ("Y", x2), ("Q", q)):
        np.save(tmp_path / f"{name}.npy", a)
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    x, y = np.stack([x1, x2], -1).astype(np.float32), q[:, OUTPUT_DIM, :, :, None].astype(np.float32)
    i, j, k = TRAIN, TRAIN + TEST, TRAIN + TEST + VALID
    splits = dict(train=dict(x=x[:i], y=y[:i]), test=dict(x=x[i:j], y=y[i:j]), valid=dict(x=x[j:k], y=y[j:k]))
    np.savez(tmp_path / "train.npz", **splits["train"])
    cfg = tmp_path / "config.yaml"
    cfg.write_text(_mesh_config())
    return str(cfg), tmp_path, splits


def _trial_files(root, trial=0):
    d = root / "checkpoints"
    tdir = d / [n for n in os.listdir(d) if n.startswith(f"trial-{trial}-")][0]
    return tdir, sorted(os.listdir(tdir))


def _split_loss(cfg_path, ckpt, split, device, batch_keys=("x", "y")):
    """The sample-weighted mean of routine.validation_step over `split` in batches of B, from the weights saved in `ckpt`."""
    from fourierflow_amd.config import build_routine, load_config
    routine = build_routine(load_config(cfg_path)).to(device)
    routine.load_lightning_model_state(str(ckpt))
    routine.to(device)
    routine.eval()
    n = len(split[batch_keys[0]])
    total = 0.0
    with torch.no_grad():
        for lo in range(0, n, B):
            batch = {k: torch.from_numpy(np.ascontiguousarray(split[k][lo:lo + B])).to(device) for k in batch_keys}
            total += float(routine.validation_step(batch).item()) * len(batch[batch_keys[0]])
    return total / n


# the file name carries five decimals (half a unit of the fifth), the log line six; the weighted mean of three float32 losses of
# order 1 accumulated in another order differs by a few 1e-7
NAME_TOL, LOG_TOL = 0.5e-5 + 1e-6, 0.5e-6 + 1e-6


def test_unshuffled_builder_run_equals_the_npz_run(mesh, host_device):
    """Four steps print every step on the npz path; the builder path prints the last step of each of its two epochs."""
    cfg, root, _ = mesh
    log_n, sum_n, state_n = _run(["train", cfg, "--data", str(root / "train.npz"), "--steps", "4", "--size", str(X), "--size", str(Y),
                                  "--no-logging"], host_device)
    log_b, sum_b, state_b = _run(["train", cfg, "--builder", "--epochs", "2", "--no-shuffle", "--checkpoint-id", "b"], host_device)
    assert [l["step"] for l in log_n] == [0, 1, 2, 3] and all(np.isfinite(l["train_loss"]) for l in log_n)
    assert [(l["epoch"], l["step"]) for l in log_b] == [(1, 2), (2, 4)]
    assert [l["train_loss"] for l in log_b] == [log_n[1]["train_loss"], log_n[3]["train_loss"]]
    assert [l["lr"] for l in log_b] == [log_n[1]["lr"], log_n[3]["lr"]]
    assert sum_b["steps"] == sum_n["steps"] == 4 and sum_b["batch"] == sum_n["batch"] == B and sum_b["epochs"] == 2
    assert set(state_b) == set(state_n) and len(state_b) > 10
    for k in state_b:
        assert state_b[k].tobytes() == state_n[k].tobytes(), k
    tdir, files = _trial_files(root)
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["epoch"] == 2 and last["global_step"] == 4
    for k, v in last["state_dict"].items():                  # the parameters in last.ckpt are the npz run's too
        if k in state_n:
            assert v.numpy().tobytes() == state_n[k].tobytes(), k
    assert len([k for k in last["state_dict"] if k in state_n]) > 10


def test_seeded_shuffle(mesh, host_device):
    cfg, _, _ = mesh
    common = ["train", cfg, "--builder", "--epochs", "2", "--no-logging"]
    log_a, _, state_a = _run(common, host_device)
    log_b, _, state_b = _run(common, host_device)                       # the same trial: the same permutations
    assert log_a == log_b
    for k in state_a:
        assert state_a[k].tobytes() == state_b[k].tobytes(), k
    log_c, _, _ = _run([*common, "--no-shuffle"], host_device)
    assert [l["train_loss"] for l in log_c] != [l["train_loss"] for l in log_a]


def test_validation_loss_best_checkpoint_and_test(mesh, host_device):
    cfg, root, splits = mesh
    log, summary, _ = _run(["train", cfg, "--builder", "--checkpoint-id", "v"], host_device)       # trainer.max_epochs = 3
    assert [l["epoch"] for l in log] == [1, 2, 3]
    tdir, files = _trial_files(root)
    assert len(files) == 2 and files[1] == "last.ckpt"
    # the best file is the epoch with the smallest valid_loss, named after it; the flags say when it was replaced
    vls = [l["valid_loss"] for l in log]
    best = int(np.argmin(vls))
    assert [l["best"] for l in log] == [all(v < u for u in vls[:e]) for e, v in enumerate(vls)]
    assert files[0].startswith(f"epoch={best + 1}-step={2 * (best + 1)}-valid_loss=")
    in_name = float(files[0].rpartition("valid_loss=")[2][:-len(".ckpt")])
    assert abs(in_name - vls[best]) <= NAME_TOL and abs(summary["valid_loss"] - vls[best]) <= LOG_TOL
    # ... and equals the sample-weighted mean of validation_step over the whole validation split (3 samples: 2 + 1)
    want = _split_loss(cfg, tdir / files[0], splits["valid"], host_device)
    assert abs(in_name - want) <= NAME_TOL, (in_name, want)
    # last.ckpt holds the last epoch's weights, whose validation loss is the last line's
    assert abs(_split_loss(cfg, tdir / "last.ckpt", splits["valid"], host_device) - vls[-1]) <= LOG_TOL
    _, t, _ = _run(["test", cfg, "--builder"], host_device)
    assert t["checkpoint"].endswith(files[0]) and t["samples"] == TEST
    assert abs(t["test_loss"] - _split_loss(cfg, tdir / files[0], splits["test"], host_device)) <= LOG_TOL


def test_an_epoch_that_does_not_improve_leaves_the_best_file(mesh, host_device):
    """At a learning rate of 0 the weights stay as they are: the later epochs validate to the SAME loss, which is no improvement
    (mode min is strict), so the file of epoch 1 stays while last.ckpt moves on."""
    cfg, root, _ = mesh
    frozen = ["train", cfg, "routine.optimizer.lr=0.0", "--builder", "--no-shuffle"]
    log, _, _ = _run([*frozen, "--epochs", "1", "--checkpoint-id", "w"], host_device)
    tdir, files = _trial_files(root)
    first = files[0]
    assert first.startswith("epoch=1-step=2-") and log[0]["best"]
    stamp = (tdir / first).read_bytes()
    log2, _, _ = _run([*frozen, "--epochs", "3", "--resume"], host_device)
    assert [l["epoch"] for l in log2] == [2, 3]                          # --resume continues from last.ckpt's epoch
    assert [l["valid_loss"] for l in log2] == [log[0]["valid_loss"]] * 2
    assert not any(l["best"] for l in log2)
    tdir, files = _trial_files(root)
    assert files == [first, "last.ckpt"] and (tdir / first).read_bytes() == stamp
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["epoch"] == 3 and last["global_step"] == 6


def test_resumed_run_equals_the_uninterrupted_one(mesh, host_device):
    cfg, root, _ = mesh
    log_full, _, state_full = _run(["train", cfg, "--builder", "--epochs", "2", "--no-logging"], host_device)
    _run(["train", cfg, "--builder", "--epochs", "1", "--checkpoint-id", "r"], host_device)
    log_res, _, state_res = _run(["train", cfg, "--builder", "--epochs", "2", "--resume"], host_device)
    assert [l["train_loss"] for l in log_res] == [log_full[1]["train_loss"]]     # the second epoch's permutation, weights and moments
    for k in state_full:
        assert state_full[k].tobytes() == state_res[k].tobytes(), k


def test_step_lr_halves_the_printed_lr_each_epoch(mesh, host_device):
    cfg, root, _ = mesh
    (root / "geo.yaml").write_text(_mesh_config(GEO_MODEL))
    log, _, _ = _run(["train", str(root / "geo.yaml"), "--builder", "--epochs", "3", "--no-logging"], host_device)
    assert [l["lr"] for l in log] == [1e-3, 5e-4, 2.5e-4]
    assert all(np.isfinite(l["train_loss"]) and np.isfinite(l["valid_loss"]) for l in log)


def test_elasticity_files_drive_the_point_cloud_routine(tmp_path, host_device, monkeypatch):
    rs = np.random.RandomState(72)
    P = 37
    rr, sigma, xy = rs.standard_normal((42, N_FILE)), rs.standard_normal((P, N_FILE)), rs.uniform(0, 1, (P, 2, N_FILE))
    for name, a in (("rr", rr), ("sigma", sigma), ("xy", xy)):
        np.save(tmp_path / f"{name}.npy", a)
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(POINTCLOUD)
    # elasticity.py:23-49: the permuted arrays; train from the front, valid [-eval:-test], test [-test:]
    full = dict(xy=np.transpose(xy, (2, 0, 1)).astype(np.float32), rr=rr.T.astype(np.float32),
                sigma=sigma.T.astype(np.float32)[..., None])
    ev = VALID + TEST
    splits = {s: {k: v[sl] for k, v in full.items()}
              for s, sl in (("train", slice(0, TRAIN)), ("valid", slice(-ev, -TEST)), ("test", slice(-TEST, None)))}
    np.savez(tmp_path / "train.npz", **splits["train"])
    log_n, _, state_n = _run(["train", str(cfg), "--data", str(tmp_path / "train.npz"), "--steps", "4", "--no-logging"], host_device)
    log_b, _, state_b = _run(["train", str(cfg), "--builder", "--no-shuffle", "--checkpoint-id", "e"], host_device)   # max_epochs = 2
    assert [l["train_loss"] for l in log_b] == [log_n[1]["train_loss"], log_n[3]["train_loss"]]
    for k in state_b:
        assert state_b[k].tobytes() == state_n[k].tobytes(), k
    tdir, files = _trial_files(tmp_path)
    keys = ("xy", "rr", "sigma")
    in_name = float(files[0].rpartition("valid_loss=")[2][:-len(".ckpt")])
    assert abs(in_name - _split_loss(str(cfg), tdir / files[0], splits["valid"], host_device, keys)) <= NAME_TOL
    _, t, _ = _run(["test", str(cfg), "--builder"], host_device)
    assert abs(t["test_loss"] - _split_loss(str(cfg), tdir / files[0], splits["test"], host_device, keys)) <= LOG_TOL


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
builder:
  _target_: fourierflow.builders.NSMarkovBuilder
  batch_size: 3
"""


def test_refusals(mesh, host_device):
    cfg, root, _ = mesh

    def refused(args, word):
        res = _invoke(args, host_device)
        assert res.exit_code != 0 and isinstance(res.exception, ValueError) and word in str(res.exception), (args, res.exception)

    refused(["train", cfg, "--builder", "--data", str(root / "train.npz"), "--no-logging"], "--data")
    refused(["train", cfg, "--builder", "--steps-per-epoch", "2", "--no-logging"], "--steps-per-epoch")
    refused(["test", cfg, "--builder", "--data", str(root / "train.npz")], "--data")
    (root / "markov.yaml").write_text(MARKOV)
    for word in ("StructuredMesh2DBuilder", "PlasticityBuilder", "ElasticityBuilder"):       # the message names the three
        refused(["train", str(root / "markov.yaml"), "--builder", "--epochs", "1", "--no-logging"], word)
    # a mesh routine whose config names the point-cloud builder (or none) is refused the same way
    refused(["train", cfg, "builder._target_=fourierflow.builders.ElasticityBuilder", "--builder", "--no-logging"], "ElasticityBuilder")
    (root / "bare.yaml").write_text(_mesh_config().split("builder:")[0])
    refused(["train", str(root / "bare.yaml"), "--builder", "--epochs", "1", "--no-logging"], "StructuredMesh2DBuilder")
