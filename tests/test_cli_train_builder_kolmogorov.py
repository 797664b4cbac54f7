"""`train | test | predict CONFIG --builder` for the Kolmogorov-flow experiments: the reference's own
torus_kochkov/ffno/ablation/ffno-nw/64/config.yaml (Grid2DMarkovExperiment with use_velocity on KolmogorovBuilder, stored in
tests/golden/reference_configs.npz), shrunk by overrides to one layer of width 32 with 4 modes on a 16 x 16 grid, k = 2, batches of 4
and two epochs (statistics + one training epoch), on files of two trajectories per split -- 16 x 16 x 9 with 8 x 8 corr trajectories
-- that the tests write as the .npz siblings of the .nc files the config names.  Emulator and GPU."""
import os

import numpy as np
import pytest
import torch

from backend_util import host_device  # noqa: F401
from test_cli_train_builder_ns import _invoke, _run, _trial_files
from test_config import shipped_configs

G, M2, TT, K, B, N = 16, 8, 9, 2, 4, 2
STEPS_PER_EPOCH = 4                                      # 2 x (9 - 2) = 14 pairs in batches of 4: 4 4 4 2
N_STEPS = 4                                              # data columns 0 2 4 6 8 of the 1 + 9 joined snapshots: four steps
OVERRIDES = ["routine.conv.n_layers=1", "routine.conv.width=32", "routine.conv.modes=4", "routine.grid_size=[16]",
             f"builder.train_dataset.k={K}", f"builder.valid_dataset.k={K}", f"builder.test_dataset.k={K}", f"builder.batch_size={B}",
             "trainer.max_epochs=2"]
VALID = ("valid_loss", "valid_loss_avg", "valid_time_until", "valid_reduced_time_until", "valid_corr")


@pytest.fixture()
def case(tmp_path, monkeypatch):
    rs = np.random.RandomState(97)
    base = tmp_path / "kolmogorov" / "re_1000"
    os.makedirs(base / "trajectories")
    os.makedirs(base / "initial_conditions")
    for split in ("train", "valid", "test"):
        w = (rs.standard_normal((N, G, G, TT)) + 0.3).astype(np.float32)
        if split == "train":
            np.savez(base / "trajectories" / "train_64_4.npz", data=w)       # the generator's layout
            continue
        np.savez(base / "trajectories" / f"{split}_64_4.npz", vorticity=np.moveaxis(w, -1, 1), time=0.28 * np.arange(1, TT + 1))
        np.savez(base / "trajectories" / f"{split}_32_4.npz", vorticity=rs.standard_normal((N, TT, M2, M2)).astype(np.float32))
        np.savez(base / "initial_conditions" / f"{split}_64.npz", vorticity=rs.standard_normal((N, G, G)).astype(np.float32))
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()["torus_kochkov/ffno/ablation/ffno-nw/64/config.yaml"])
    return str(cfg), tmp_path


def _best(scores, start=-np.inf):
    """(best score, 1-based epochs that improved on it strictly) of a max monitor."""
    best, improved = start, []
    for e, s in enumerate(scores, 1):
        if s > best:
            best, improved = s, improved + [e]
    return best, improved


def test_train_selects_by_the_configs_checkpoint_entry_then_test_and_predict(case, host_device):
    from fourierflow_amd.cli import _last_routine
    cfg, root = case
    log, summary, state, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--checkpoint-id", "k"], host_device)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, STEPS_PER_EPOCH)] and summary["epochs"] == 2
    assert log[0]["train_loss"] is None and np.isfinite(log[1]["train_loss"])
    for line in log:
        assert set(VALID) <= set(line) and all(np.isfinite(line[k]) for k in VALID)
    routine = _last_routine()
    assert routine.downsample_corr and routine.use_velocity
    assert routine.last_metrics.numel() == (4 + 2 * N_STEPS) + (2 + N_STEPS)      # the reduced numbers came in the same read
    best, improved = _best([l["valid_time_until"] for l in log])
    assert [l["best"] for l in log] == [e in improved for e in (1, 2)]
    tdir, names = _trial_files(root)
    e = improved[-1]
    want = f"epoch={e}-step={log[e - 1]['step']}-valid_time_until={log[e - 1]['valid_time_until']:.3f}.ckpt"
    assert names == [want, "last.ckpt"], names
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["callbacks"]["ModelCheckpoint"]["monitor"] == "valid_time_until"
    assert abs(last["callbacks"]["ModelCheckpoint"]["best_model_score"] - best) <= 1e-6 and abs(summary["valid_time_until"] - best) <= 1e-6
    # test --builder: the test files, from that checkpoint, with the reduced time
    _, t, _, _ = _run(["test", cfg, *OVERRIDES, "--builder"], host_device)
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr", "test_reduced_time_until", "samples"}
    assert t["samples"] == N and t["checkpoint"].endswith(want) and np.isfinite(t["test_reduced_time_until"])
    # predict --builder: the joined test trajectories at every k-th time
    _, p, _, _ = _run(["predict", cfg, *OVERRIDES, "--builder"], host_device)
    assert p["shape"] == [N, G, G, N_STEPS] and p["samples"] == N and p["n_steps"] == N_STEPS and p["inference_time"] > 0


def test_resume_continues_with_the_stored_best_score(case, host_device):
    cfg, root = case
    log, _, _, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "1", "--checkpoint-id", "r"], host_device)
    tdir, names = _trial_files(root)
    assert len(names) == 2 and names[0].startswith("epoch=1-step=0-valid_time_until=")
    # a stored score no epoch can beat: the resumed run must keep the first file
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert abs(last["callbacks"]["ModelCheckpoint"]["best_model_score"] - log[0]["valid_time_until"]) <= 1e-6
    last["callbacks"]["ModelCheckpoint"]["best_model_score"] = 1e9
    torch.save(last, tdir / "last.ckpt")
    log2, summary2, _, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "2", "--resume"], host_device)
    assert [(l["epoch"], l["step"], l["best"]) for l in log2] == [(2, STEPS_PER_EPOCH, False)]
    assert summary2["valid_time_until"] == 1e9 and _trial_files(root)[1] == names
    again = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert again["epoch"] == 2 and again["callbacks"]["ModelCheckpoint"]["best_model_score"] == 1e9
    # ... and without a stored score the monitor starts from -inf: the first resumed epoch is the best so far
    del again["callbacks"]
    torch.save(again, tdir / "last.ckpt")
    log3, _, _, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "3", "--resume"], host_device)
    assert [(l["epoch"], l["best"]) for l in log3] == [(3, True)]
    assert _trial_files(root)[1][0].startswith("epoch=3-step=8-valid_time_until=")


def test_other_builders_keep_valid_loss_min(case):
    from fourierflow_amd.cli import _checkpoint_rule

    class NSMarkovBuilder:
        pass

    cfg = {"callbacks": [{"_target_": "fourierflow.callbacks.CustomModelCheckpoint", "monitor": "valid_time_until", "mode": "max"}]}
    assert _checkpoint_rule(cfg, NSMarkovBuilder()) == ("valid_loss", "min", None)


def test_a_missing_npz_sibling_refuses_the_command_with_the_one_message(case, host_device):
    cfg, root = case
    os.remove(root / "kolmogorov" / "re_1000" / "trajectories" / "valid_32_4.npz")
    res = _invoke(["train", cfg, *OVERRIDES, "--builder", "--no-logging"], host_device)
    assert res.exit_code != 0 and isinstance(res.exception, FileNotFoundError), (res.output, res.exception)
    for word in ("valid_32_4.npz", "netCDF is not read", "xarray.open_dataset", "generate navier-stokes"):
        assert word in str(res.exception), (word, res.exception)
