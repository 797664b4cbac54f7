"""`train | test | predict CONFIG --builder` for the contextual Navier-Stokes experiments: the reference's own
torus_vis_force/01_baseline/config.yaml (Grid2DMarkovExperiment with append_force and append_mu on NSContextualBuilder, stored in
tests/golden/reference_configs.npz), shrunk by overrides to one layer of width 32 with 4 modes, n_steps = 2, k = 2, ssr = 1 and
batches of 4, on files of three (train) and two (valid, test) trajectories of 16 x 16 x 7 that the tests write where the config
looks for its HDF5 file.  Once with one force map per trajectory and once with one per snapshot.  Emulator and GPU."""
import os

import numpy as np
import pytest
import torch

from backend_util import host_device  # noqa: F401
from test_cli_train_builder_ns import LOG_TOL, _fresh, _invoke, _run, _same_state, _state, _trial_files, _weighted
from test_config import shipped_configs

G, T, K, B = 16, 7, 2, 4
N = dict(train=3, valid=2, test=2)                      # 3 x (7 - 2) = 15 pairs: four steps an epoch (4 4 4 3)
STEPS_PER_EPOCH = 4
OVERRIDES = ["routine.conv.n_layers=1", "routine.conv.width=32", "routine.conv.modes=4", "routine.n_steps=2", f"builder.k={K}",
             "builder.ssr=1", f"builder.batch_size={B}"]
QUIET = OVERRIDES + ["routine.noise_std=0.0"]            # for runs that are compared with one another step by step
VALID = ("valid_loss", "valid_loss_avg", "valid_time_until", "valid_reduced_time_until", "valid_corr")


@pytest.fixture(params=["const", "step"])
def case(request, tmp_path, monkeypatch):
    """(config path, root, {split: arrays}) with the three files at ${DATA_ROOT}/torus/torus_vis_force.{train,valid,test}.npz."""
    rs = np.random.RandomState(93 + (request.param == "step"))
    os.makedirs(tmp_path / "torus")
    arrays = {}
    for split, n in N.items():
        u = (rs.standard_normal((n, G, G, T)) + 0.3).astype(np.float32)
        f = rs.standard_normal((n, G, G, T) if request.param == "step" else (n, G, G)).astype(np.float32)
        mu = rs.uniform(1e-5, 1e-3, n).astype(np.float32)
        np.savez(tmp_path / "torus" / f"torus_vis_force.{split}.npz", data=u, f=f, mu=mu)
        arrays[split] = dict(u=u, f=f, mu=mu)
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()["torus_vis_force/01_baseline/config.yaml"])
    return str(cfg), tmp_path, arrays


def _held_out_batches(a, device):
    """The batches of NavierStokesDataset (ns_contextual.py:91-101) over a split that fits one batch."""
    f = a["f"][..., ::K] if a["f"].ndim == 4 else a["f"]
    times = np.tile(np.arange(0, 20, 0.1 * K).astype(np.float32), (len(a["u"]), 1))
    host = dict(data=a["u"][..., ::K], f=f, mu=a["mu"], times=times)
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}]


def test_the_builder_section_instantiates(case):
    from fourierflow_amd.builders import NSContextualBuilder
    from fourierflow_amd.config import instantiate, load_config
    cfg_path, root, arrays = case
    bld = instantiate(load_config(cfg_path, OVERRIDES)["builder"])
    assert isinstance(bld, NSContextualBuilder) and (bld.ssr, bld.k, bld.batch_size) == (1, K, B)
    assert bld.files["train"] == str(root / "torus" / "torus_vis_force.train.npz")
    assert bld.arrays("valid")["f"].shape == arrays["valid"]["f"].shape
    shipped = instantiate(load_config(cfg_path)["builder"])            # ... and as shipped: ssr = 4, k = 10, batch 19
    assert (shipped.ssr, shipped.k, shipped.batch_size) == (4, 10, 19)


def test_statistics_epoch_then_training_epoch_through_resume(case, host_device):
    cfg, root, _ = case
    log, summary, state, (m, v) = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "1", "--checkpoint-id", "c"], host_device)
    assert [(l["epoch"], l["step"], l["train_loss"]) for l in log] == [(1, 0, None)] and summary["steps"] == 0
    assert summary["batch"] == B and np.isfinite(log[0]["valid_loss"]) and set(VALID) <= set(log[0])
    initial = _state(_fresh(cfg, host_device, OVERRIDES))
    changed = [k for k in state if state[k].tobytes() != initial[k].tobytes()]
    assert changed and all(k.startswith("normalizer.") for k in changed), changed      # epoch 0: the statistics and no parameter
    assert not m.any() and not v.any()
    # every pair once; five feature channels (x, two positions, force, mu) pooled over the grid
    assert state["normalizer.count"] == N["train"] * (T - K) * G * G and state["normalizer.n_accumulations"] == STEPS_PER_EPOCH
    tdir, names = _trial_files(root)
    assert len(names) == 2 and names[0].startswith("epoch=1-step=0-valid_loss=") and names[1] == "last.ckpt"
    # --resume continues with epoch 1, the first that optimises
    log2, summary2, state2, (m2, _) = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "2", "--resume"], host_device)
    assert [(l["epoch"], l["step"]) for l in log2] == [(2, STEPS_PER_EPOCH)] and np.isfinite(log2[0]["train_loss"])
    assert summary2["resumed_from_step"] == 0 and summary2["steps"] == STEPS_PER_EPOCH and np.isfinite(log2[0]["valid_loss"])
    moved = [k for k in state2 if not k.startswith("normalizer.") and state2[k].tobytes() != state[k].tobytes()]
    assert len(moved) >= 10 and m2.any()                               # epoch 1 changes the parameters
    assert state2["normalizer.n_accumulations"] == 2 * STEPS_PER_EPOCH
    tdir, names = _trial_files(root)
    assert names[-1] == "last.ckpt" and len(names) == 2 and names[0].startswith("epoch=")
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["epoch"] == 2 and last["global_step"] == STEPS_PER_EPOCH


def test_epochs_equal_the_hand_written_loop_and_validation_the_whole_split(case, host_device):
    """The unshuffled run against MarkovTrajectoryData fed by hand (a per-step force gives each pair the map of its target time),
    the logged validation keys against validation_step on the reference's held-out batch, and `test --builder`."""
    from fourierflow_amd.builders import MarkovTrajectoryData
    cfg, root, arrays = case
    log, summary, state, _ = _run(["train", cfg, *QUIET, "--builder", "--epochs", "2", "--no-shuffle", "--checkpoint-id", "h"], host_device)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, STEPS_PER_EPOCH)] and summary["epochs"] == 2
    routine = _fresh(cfg, host_device, QUIET)
    a = arrays["train"]
    ds = MarkovTrajectoryData(a["u"], a["f"], a["mu"], device=host_device, batch_size=B, mode="kolmogorov", k=K, seed=0, shuffle=False)
    losses = [routine.training_step(batch, epoch=epoch) for epoch in range(2) for batch in ds.epoch()]
    assert losses[:STEPS_PER_EPOCH] == [None] * STEPS_PER_EPOCH
    _same_state(state, _state(routine))
    assert log[-1]["train_loss"] == round(float(losses[-1].item()), 6)
    want = _weighted(routine, _held_out_batches(arrays["valid"], host_device))
    assert set(want) == set(VALID)
    for k in VALID:
        assert abs(log[-1][k] - want[k]) <= LOG_TOL, (k, log[-1][k], want[k])
    # test --builder: the test file, from the best checkpoint
    tdir, names = _trial_files(root)
    _, t, _, _ = _run(["test", cfg, *QUIET, "--builder"], host_device)
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr", "samples"}
    assert t["samples"] == N["test"] and t["checkpoint"].endswith(names[0])
    assert np.isfinite(t["test_loss"]) and np.isfinite(t["test_time_until"])
    routine.load_lightning_model_state(str(tdir / names[0]))
    routine.to(host_device)
    want = _weighted(routine, _held_out_batches(arrays["test"], host_device), "test_step")
    for k in ("test_loss", "test_loss_avg", "test_time_until", "test_corr"):
        assert abs(t[k] - want[k]) <= LOG_TOL, (k, t[k], want[k])


def test_predict_is_refused(case, host_device):
    cfg, _, _ = case
    _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "1", "--checkpoint-id", "p"], host_device)
    res = _invoke(["predict", cfg, *OVERRIDES, "--builder"], host_device)
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
    for word in ("NSContextualBuilder", "inference_data()", "reference", "test --builder"):
        assert word in str(res.exception), (word, res.exception)


def test_missing_files_refuse_the_command_with_the_one_message(case, host_device):
    cfg, root, _ = case
    os.remove(root / "torus" / "torus_vis_force.valid.npz")
    res = _invoke(["train", cfg, *OVERRIDES, "--builder", "--epochs", "1", "--no-logging"], host_device)
    assert res.exit_code != 0 and isinstance(res.exception, FileNotFoundError), (res.output, res.exception)
    for word in ("torus_vis_force.valid.npz", "generate navier-stokes", "--train-trajectories"):
        assert word in str(res.exception), (word, res.exception)
