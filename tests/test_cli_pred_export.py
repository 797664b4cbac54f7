"""`test CONFIG --builder [--pred-path P]` with a Markov routine that has a ``pred_path``: the predictions of the WHOLE test split go
into one file (reference routines/grid_2d_markov.py:427-476 overwrites its file with every batch).  The pattern, the shrunk
torus_kochkov config and the file layout are those of tests/test_cli_train_builder_kolmogorov.py; the test split holds three
trajectories and is read in batches of two, so that a short last batch is part of it.  pred_size = 8 on the 16 x 16 model.
Emulator and GPU."""
import os

import numpy as np
import pytest

from backend_util import host_device  # noqa: F401
from test_cli_train_builder_kolmogorov import G, M2, N, N_STEPS, OVERRIDES, TT
from test_cli_train_builder_ns import _invoke, _run
from test_config import shipped_configs

N_TEST, PRED = 3, 8
TODAY = {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr", "test_reduced_time_until", "samples"}
PREDICTIONS = [f"torus_kochkov/ffno/predictions/{g}/config.yaml" for g in (64, 128, 256)]


@pytest.fixture()
def case(tmp_path, monkeypatch):
    rs = np.random.RandomState(98)
    base = tmp_path / "kolmogorov" / "re_1000"
    os.makedirs(base / "trajectories")
    os.makedirs(base / "initial_conditions")
    for split, n in (("train", N), ("valid", N), ("test", N_TEST)):
        w = (rs.standard_normal((n, G, G, TT)) + 0.3).astype(np.float32)
        if split == "train":
            np.savez(base / "trajectories" / "train_64_4.npz", data=w)
            continue
        np.savez(base / "trajectories" / f"{split}_64_4.npz", vorticity=np.moveaxis(w, -1, 1), time=0.28 * np.arange(1, TT + 1))
        np.savez(base / "trajectories" / f"{split}_32_4.npz", vorticity=rs.standard_normal((n, TT, M2, M2)).astype(np.float32))
        np.savez(base / "initial_conditions" / f"{split}_64.npz", vorticity=rs.standard_normal((n, G, G)).astype(np.float32))
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()["torus_kochkov/ffno/ablation/ffno-nw/64/config.yaml"])
    return str(cfg), tmp_path


def test_test_builder_writes_one_file_for_the_whole_split(case, host_device):
    cfg, root = case
    _run(["train", cfg, *OVERRIDES, "--builder", "--checkpoint-id", "p"], host_device)
    # without a pred_path: exactly today's keys, and no file
    _, plain, _, _ = _run(["test", cfg, *OVERRIDES, "--builder", "--batch-size", "2"], host_device)
    assert set(plain) == TODAY and plain["samples"] == N_TEST
    assert not [f for _, _, fs in os.walk(root) for f in fs if f.startswith("preds")]
    # routine.pred_path by override, as the predictions configs set it
    target = root / "out" / "nested" / "preds.nc"
    _, t, _, _ = _run(["test", cfg, *OVERRIDES, f"routine.pred_path={target}", f"routine.pred_size={PRED}", "--builder",
                       "--batch-size", "2"], host_device)
    written = str(root / "out" / "nested" / "preds.npz")
    assert set(t) == TODAY | {"pred_path", "pred_samples"}
    assert t["pred_path"] == written and t["pred_samples"] == N_TEST == t["samples"]
    assert {k: t[k] for k in TODAY} == plain      # the export moves no metric
    assert os.listdir(root / "out" / "nested") == ["preds.npz"]
    with np.load(written) as z:
        for name in ("vorticity", "vx", "vy"):      # three samples from batches of 2 and 1
            assert z[name].shape == (N_TEST, PRED, PRED, N_STEPS) and z[name].dtype == np.float32 and np.isfinite(z[name]).all()
        assert z["energy_spectrum"].shape == (N_TEST, N_STEPS, PRED // 2 + 1) and (z["energy_spectrum"] >= 0).all()
        assert z["time"].shape == (N_STEPS,) and np.all(np.diff(z["time"]) > 0)
        np.testing.assert_allclose(z["x"], (np.arange(PRED) + 0.5) * 2 * np.pi / PRED, rtol=1e-12)
        first = {name: z[name].copy() for name in ("vorticity", "vx", "energy_spectrum")}
        # Parseval on the written arrays: the shells inside the circle hold at most the mean kinetic energy
        ke = ((z["vx"].astype(np.float64) ** 2 + z["vy"].astype(np.float64) ** 2) / 2).mean(axis=(1, 2))      # [sample, time]
        assert (z["energy_spectrum"].sum(-1) <= ke * (1 + 1e-5)).all() and (z["energy_spectrum"].sum(-1) > 0).all()
    # --pred-path overrides the routine's; one batch for the whole split gives the same samples in the same order
    other = root / "elsewhere.npz"
    _, o, _, _ = _run(["test", cfg, *OVERRIDES, f"routine.pred_path={target}", f"routine.pred_size={PRED}", "--builder",
                       "--pred-path", str(other)], host_device)
    assert o["pred_path"] == str(other) and o["pred_samples"] == N_TEST
    with np.load(other) as z:
        for name, a in first.items():
            assert np.array_equal(z[name], a), name


def test_pred_path_needs_the_markov_trajectory_rollout(case, host_device):
    cfg, root = case
    _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "1", "--checkpoint-id", "q"], host_device)
    res = _invoke(["test", cfg, *OVERRIDES, "--pred-path", str(root / "p.npz")], host_device)      # synthetic one-step pairs
    assert res.exit_code != 0 and isinstance(res.exception, ValueError) and "--data TRAJ.npz" in str(res.exception)
    assert not os.path.exists(root / "p.npz")


@pytest.mark.parametrize("rel", PREDICTIONS)
def test_shipped_predictions_configs_build_with_pred_path_on_the_routine(rel, tmp_path):
    import yaml

    from fourierflow_amd.config import build_routine, load_config
    text = shipped_configs()[rel]
    path = tmp_path / "config.yaml"
    path.write_text(text)
    routine = build_routine(load_config(str(path), []))
    want = yaml.safe_load(text)["routine"]["pred_path"]
    assert want.endswith("preds.nc") and routine.pred_path == want and routine.pred_size == 64
    assert routine.use_velocity and routine.conv.n_layers == 24
