"""`generate navier-stokes PATH --force random --varying-force`: the files carry one force map per snapshot (f [n, M, N, steps]
beside `data`; in the x / y form of the training file the map of each pair's target), the same seed writes the same bytes, and
the reference's own torus_vis_force/01_baseline config (tests/golden/reference_configs.npz, shrunk by the overrides of
test_cli_train_builder_contextual.py) trains and tests on them through NSContextualBuilder.  Grid 16, t = 1 at delta = 1e-2
(100 solver steps), 5 snapshots, t_scaling = 5: the phase moves one radian from snapshot to snapshot."""
import json

import numpy as np
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401
from test_cli_train_builder_ns import _fresh, _run as _run_train, _state
from test_config import shipped_configs

S, STEPS, N_TRAIN, N_HELD = 16, 5, 4, 2
ARGS = ["--s", str(S), "--t", "1", "--delta", "1e-2", "--steps", str(STEPS), "--batch-size", "2", "--seed", "11", "--n-train",
        str(N_TRAIN), "--n-valid", str(N_HELD), "--n-test", str(N_HELD), "--force", "random", "--varying-force", "--t-scaling", "5",
        "--mu-min", "1e-4", "--mu-max", "1e-3"]
OVERRIDES = ["routine.conv.n_layers=1", "routine.conv.width=32", "routine.conv.modes=4", "routine.n_steps=2", "builder.k=2",
             "builder.ssr=1", "builder.batch_size=4"]


def _generate(prefix, device, *more):
    from fourierflow_amd.cli import app
    res = CliRunner().invoke(app, ["generate", "navier-stokes", str(prefix), *ARGS, *more, "--device", device])
    assert res.exit_code == 0, (res.output, res.exception)
    summary = [json.loads(l) for l in res.output.splitlines() if l.startswith("{")][-1]
    return summary, {split: dict(np.load(f"{prefix}.{split}.npz")) for split in ("train", "valid", "test")}


def _rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64))


def test_generate_varying_force_then_train_on_it(tmp_path, host_device, monkeypatch):
    prefix = tmp_path / "torus" / "torus_vis_force"
    summary, z = _generate(prefix, host_device, "--train-trajectories")
    assert summary["varying_force"] is True and summary["t_scaling"] == 5.0 and summary["solver_steps"] == 100
    for split, n in (("train", N_TRAIN), ("valid", N_HELD), ("test", N_HELD)):
        assert {k: v.shape for k, v in z[split].items()} == dict(data=(n, S, S, STEPS), times=(n, STEPS), f=(n, S, S, STEPS), mu=(n,))
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for zz in z.values() for v in zz.values())
    f = z["train"]["f"]
    for i in range(STEPS - 1):                     # the force moves from snapshot to snapshot, and differs between trajectories
        assert _rel(f[..., i + 1], f[..., i]) > 0.1
    assert _rel(f[1], f[0]) > 0.1

    # the x / y form of the same seed: the same trajectories as pairs, each with the force map of its target
    summary, pairs = _generate(tmp_path / "pairs", host_device)
    n_pairs = N_TRAIN * (STEPS - 1)
    tr = pairs["train"]
    assert {k: v.shape for k, v in tr.items()} == dict(x=(n_pairs, S, S, 1), y=(n_pairs, S, S, 1), f=(n_pairs, S, S), mu=(n_pairs,))
    assert summary["train"]["f"] == [n_pairs, S, S] and tr["f"].dtype == np.float32
    for b in range(N_TRAIN):
        for t in range(STEPS - 1):
            row = b * (STEPS - 1) + t
            np.testing.assert_array_equal(tr["x"][row, ..., 0], z["train"]["data"][b, ..., t])
            np.testing.assert_array_equal(tr["y"][row, ..., 0], z["train"]["data"][b, ..., t + 1])
            np.testing.assert_array_equal(tr["f"][row], f[b, ..., t + 1])
    for split in ("valid", "test"):
        for k, v in z[split].items():
            np.testing.assert_array_equal(v, pairs[split][k])

    # the same seed writes the same bytes (of every array: the zip directory of an .npz carries the time of writing)
    _, again = _generate(tmp_path / "again", host_device, "--train-trajectories")
    for split, arrays in z.items():
        assert set(arrays) == set(again[split])
        for k, v in arrays.items():
            assert v.tobytes() == again[split][k].tobytes(), (split, k)

    # the reference's torus_vis_force config on the generated files
    from fourierflow_amd.builders import NSContextualBuilder
    from fourierflow_amd.config import instantiate, load_config
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()["torus_vis_force/01_baseline/config.yaml"])
    overrides = OVERRIDES + [f"builder.data_path={prefix}"]
    bld = instantiate(load_config(str(cfg), overrides)["builder"])
    assert isinstance(bld, NSContextualBuilder) and bld.arrays("train")["f"].shape == (N_TRAIN, S, S, STEPS)
    np.testing.assert_array_equal(bld.arrays("valid")["f"], z["valid"]["f"])
    log, done, state, (m, _) = _run_train(["train", str(cfg), *overrides, "--builder", "--epochs", "2", "--checkpoint-id", "v"], host_device)
    steps_per_epoch = -(-N_TRAIN * (STEPS - 2) // 4)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, steps_per_epoch)] and done["steps"] == steps_per_epoch
    assert log[0]["train_loss"] is None and np.isfinite(log[1]["train_loss"]) and all(np.isfinite(l["valid_loss"]) for l in log)
    initial = _state(_fresh(str(cfg), host_device, overrides))
    moved = [k for k in state if not k.startswith("normalizer.") and state[k].tobytes() != initial[k].tobytes()]
    assert len(moved) >= 10 and m.any()                      # epoch 1 changes the parameters
    _, t, _, _ = _run_train(["test", str(cfg), *overrides, "--builder"], host_device)
    assert t["samples"] == N_HELD and np.isfinite(t["test_loss"]) and np.isfinite(t["test_time_until"])


def test_varying_force_goes_with_the_random_force(tmp_path, host_device):
    from fourierflow_amd.cli import app
    for more in (["--force", "li"], ["--force", "random", "--cycles", str(S // 2)]):
        res = CliRunner().invoke(app, ["generate", "navier-stokes", str(tmp_path / "bad"), "--s", str(S), "--varying-force", *more,
                                       "--device", host_device])
        assert res.exit_code == 2 and "Invalid value" in res.output, (res.output, res.exception)
        assert not list(tmp_path.iterdir())
