"""`train | test | predict CONFIG --builder` for the multi-resolution Kolmogorov-flow experiments: the reference's own
torus_kochkov/ffno/multi_resolution/x32_x64/config.yaml (tests/golden/reference_configs.npz) with the one override that selects
this project's training set, builder.train_dataset._target_=fourierflow_amd.builders.KolmogorovMultiResolutionDataset, shrunk by
overrides to one layer of width 32 with 4 modes, k = 2 and batches of 4.  The files the tests write stand in for the config's: the
"64" files hold 16 x 16 grids, the "32" files 8 x 8 -- two trajectories of 9 snapshots per split, so 14 pairs in batches 4 4 4 2.  The
config's four loader workers would draw all four from the first file; builder.num_workers=1 makes them alternate 16 8 16 8.
Emulator and GPU; the two-rank run on the emulator over gloo."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from typer.testing import CliRunner

from backend_util import host_device  # noqa: F401
from test_cli_train_builder_ns import _invoke, _run, _same_state, _trial_files
from test_config import shipped_configs

FINE, COARSE, TT, K, B, N = 16, 8, 9, 2, 4, 2
STEPS_PER_EPOCH = 4                                      # 2 x (9 - 2) = 14 pairs in batches of 4: 4 4 4 2
N_STEPS = 4
MULTI = "fourierflow_amd.builders.KolmogorovMultiResolutionDataset"
OVERRIDES = [f"builder.train_dataset._target_={MULTI}",
             "routine.conv.n_layers=1", "routine.conv.width=32", "routine.conv.modes=4", f"routine.grid_size=[{COARSE},{FINE}]",
             f"builder.train_dataset.k={K}", f"builder.valid_dataset.k={K}", f"builder.test_dataset.k={K}", f"builder.batch_size={B}",
             f"builder.train_dataset.batch_size={B}", "builder.num_workers=1", "trainer.max_epochs=2",
             "routine.noise_std=0.0"]      # (the noise samples come from torch's global stream, which a resumed run starts afresh)
VALID = ("valid_loss", "valid_loss_avg", "valid_time_until", "valid_reduced_time_until", "valid_corr")
CONFIG = "torus_kochkov/ffno/multi_resolution/x32_x64/config.yaml"


def _write_case(root):
    rs = np.random.RandomState(97)
    base = root / "kolmogorov" / "re_1000"
    os.makedirs(base / "trajectories")
    os.makedirs(base / "initial_conditions")
    np.savez(base / "trajectories" / "train_64_4.npz", data=(rs.standard_normal((N, FINE, FINE, TT)) + 0.3).astype(np.float32))
    np.savez(base / "trajectories" / "train_32_4.npz",
             vorticity=(rs.standard_normal((N, TT, COARSE, COARSE)) + 0.3).astype(np.float32))
    for split in ("valid", "test"):
        w = (rs.standard_normal((N, FINE, FINE, TT)) + 0.3).astype(np.float32)
        np.savez(base / "trajectories" / f"{split}_64_4.npz", vorticity=np.moveaxis(w, -1, 1), time=0.28 * np.arange(1, TT + 1))
        np.savez(base / "trajectories" / f"{split}_32_4.npz", vorticity=rs.standard_normal((N, TT, COARSE, COARSE)).astype(np.float32))
        np.savez(base / "initial_conditions" / f"{split}_64.npz", vorticity=rs.standard_normal((N, FINE, FINE)).astype(np.float32))
    cfg = root / "config.yaml"
    cfg.write_text(shipped_configs()[CONFIG])
    return str(cfg)


@pytest.fixture()
def case(tmp_path, monkeypatch):
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    return _write_case(tmp_path), tmp_path


def test_train_two_epochs_then_test_and_predict(case, host_device):
    from fourierflow_amd.builders import MultiResolutionMarkovData
    from fourierflow_amd.cli import _last_routine
    cfg, root = case
    # epoch 0 is the statistics epoch over all batches, both sizes: no optimiser step
    log, summary, _, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "2", "--checkpoint-id", "m"], host_device)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, STEPS_PER_EPOCH)] and summary["epochs"] == 2
    assert summary["steps"] == STEPS_PER_EPOCH and summary["batch"] == B
    assert log[0]["train_loss"] is None and np.isfinite(log[1]["train_loss"])
    for line in log:
        assert set(VALID) <= set(line) and all(np.isfinite(line[k]) for k in VALID)
    routine = _last_routine()
    assert routine.downsample_corr and routine.use_velocity and float(routine.normalizer.n_accumulations) == 2 * STEPS_PER_EPOCH
    assert float(routine.normalizer.count) == 2 * (2 * B * FINE ** 2 + B * COARSE ** 2 + 2 * COARSE ** 2)
    # the workspaces of a run: both training sizes, the short last batch, the validation batch (two trajectories at the fine size)
    geometries = {k[:3] for k in routine.trainer().engine._ws_cache}
    assert geometries == {(B, (FINE, FINE), True), (B, (COARSE, COARSE), True), (2, (COARSE, COARSE), True), (N, (FINE, FINE), False)}
    # the best file is selected and named by the config's CustomModelCheckpoint entry: valid_time_until, max
    tdir, names = _trial_files(root)
    scores = [l["valid_time_until"] for l in log]
    e = 2 if scores[1] > scores[0] else 1
    want = f"epoch={e}-step={log[e - 1]['step']}-valid_time_until={scores[e - 1]:.3f}.ckpt"
    assert names == [want, "last.ckpt"] and [l["best"] for l in log] == [True, e == 2]
    last = torch.load(tdir / "last.ckpt", map_location="cpu", weights_only=False)
    assert last["callbacks"]["ModelCheckpoint"]["monitor"] == "valid_time_until" and last["epoch"] == 2
    # test --builder and predict --builder: the fine test files, as without the override
    _, t, _, _ = _run(["test", cfg, *OVERRIDES, "--builder"], host_device)
    assert set(t) == {"checkpoint", "test_loss", "test_loss_avg", "test_time_until", "test_corr", "test_reduced_time_until", "samples"}
    assert t["samples"] == N and t["checkpoint"].endswith(names[0]) and np.isfinite(t["test_reduced_time_until"])
    _, p, _, _ = _run(["predict", cfg, *OVERRIDES, "--builder"], host_device)
    assert p["shape"] == [N, FINE, FINE, N_STEPS] and p["samples"] == N and p["n_steps"] == N_STEPS
    # the set the command trained from
    from fourierflow_amd.cli import _instantiate_builder
    from fourierflow_amd.config import load_config
    bld = _instantiate_builder(load_config(cfg, OVERRIDES), "markov", None)
    data = bld.train_data(host_device, seed=7231, shuffle=False)
    assert isinstance(data, MultiResolutionMarkovData) and data.sizes == [(FINE, FINE), (COARSE, COARSE)] and data.stride == 1
    assert [tuple(b["x"].shape[:2]) for b in data.epoch()] == [(4, FINE), (4, COARSE), (4, FINE), (2, COARSE)]


def test_resume_continues_with_the_third_epochs_permutation(case, host_device):
    """Statistics epoch + one epoch, then --resume for the third: the numbers of an uninterrupted run of three epochs (from a copy of
    the config, which has its own checkpoints directory), whose step count ends at 2 x batches per epoch."""
    cfg, root = case
    os.makedirs(root / "whole")
    shutil.copy(cfg, root / "whole" / "config.yaml")
    log_w, _, state_w, moments_w = _run(["train", str(root / "whole" / "config.yaml"), *OVERRIDES, "--builder", "--epochs", "3",
                                         "--no-logging"], host_device)
    assert [(l["epoch"], l["step"]) for l in log_w] == [(1, 0), (2, STEPS_PER_EPOCH), (3, 2 * STEPS_PER_EPOCH)]
    _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "2", "--checkpoint-id", "r"], host_device)
    log_r, summary_r, state_r, moments_r = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "3", "--resume"], host_device)
    assert [(l["epoch"], l["step"]) for l in log_r] == [(3, 2 * STEPS_PER_EPOCH)] and summary_r["resumed_from_step"] == STEPS_PER_EPOCH
    assert {k: v for k, v in log_r[0].items() if k != "best"} == {k: v for k, v in log_w[2].items() if k != "best"}
    _same_state(state_w, state_r)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(moments_w, moments_r))
    assert _trial_files(root)[1][-1] == "last.ckpt"


def test_no_shuffle_and_drop_last(case, host_device):
    cfg, _ = case
    log, summary, _, _ = _run(["train", cfg, *OVERRIDES, "--builder", "--epochs", "2", "--no-shuffle", "--drop-last", "--no-logging"],
                              host_device)
    assert [(l["epoch"], l["step"]) for l in log] == [(1, 0), (2, STEPS_PER_EPOCH - 1)] and summary["steps"] == STEPS_PER_EPOCH - 1


def test_without_the_override_the_command_names_the_dataset(case, host_device):
    cfg, _ = case
    res = _invoke(["train", cfg, *OVERRIDES[1:], "--builder", "--no-logging"], host_device)
    assert res.exit_code != 0 and isinstance(res.exception, NotImplementedError), (res.output, res.exception)
    assert "fourierflow.builders.KolmogorovMultiTorchDataset is not built" in str(res.exception) and MULTI in str(res.exception)


def test_a_batch_size_flag_that_splits_the_two_is_refused(case, host_device):
    cfg, _ = case
    res = _invoke(["train", cfg, *OVERRIDES, "--builder", "--batch-size", "3", "--no-logging"], host_device)
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
    assert "train_dataset.batch_size = 4 but the builder's batch_size = 3" in str(res.exception)


def _ddp_worker(rank, world, port, root):
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), FFNO_ALLOW_TEST_BACKEND="1", DATA_ROOT=root)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from backend_util import emu_lib
    from fourierflow_amd import _lib
    _lib._install_test_backend(emu_lib())
    from fourierflow_amd.cli import _last_routine, app
    res = CliRunner().invoke(app, ["train", os.path.join(root, "config.yaml"), *OVERRIDES, "--builder", "--epochs", "2",
                                   "--device", "cpu"])
    assert res.exit_code == 0, (res.output, res.exception)
    lines = [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]
    assert (len(lines) > 0) == (rank == 0)
    routine = _last_routine()
    sd = {k: v.detach().cpu().numpy() for k, v in routine.state_dict().items() if not np.iscomplexobj(v.detach().cpu().numpy())}
    np.savez(os.path.join(root, f"rank{rank}.npz"), steps=np.array(routine.trainer().step_count), **sd)
    if rank == 0:
        with open(os.path.join(root, "log.json"), "w") as f:
            json.dump(lines, f)
    torch.distributed.destroy_process_group()


def test_two_ranks_step_the_same_sizes_and_end_equal(tmp_path):
    """Two spawned processes, gloo, the CPU emulator: of the four batches 16 8 16 8 rank r takes batches r and r + 2 -- drawn at its
    own positions 0 and 1, i.e. at 16 and 8 on both ranks -- gradients are all-reduced per step, and both ranks end bit-identical."""
    import torch.multiprocessing as mp
    _write_case(tmp_path)
    port = 29600 + ((os.getpid() + 977) % 2000)
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert int(r0["steps"]) == int(r1["steps"]) == STEPS_PER_EPOCH // 2
    assert set(r0.files) == set(r1.files) and len(r0.files) > 10
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)
    with open(tmp_path / "log.json") as f:
        lines = json.load(f)
    assert [(l["epoch"], l["step"]) for l in lines[:-1]] == [(1, 0), (2, STEPS_PER_EPOCH // 2)] and lines[-1]["world_size"] == 2
    tdirs = os.listdir(tmp_path / "checkpoints")
    assert len(tdirs) == 1 and "last.ckpt" in os.listdir(tmp_path / "checkpoints" / tdirs[0])
