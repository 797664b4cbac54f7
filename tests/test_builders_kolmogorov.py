"""KolmogorovBuilder with KolmogorovTorchDataset / KolmogorovTrajectoryDataset (fourierflow_amd/builders/kolmogorov.py; reference
builders/kolmogorov.py:30-68, 111-139, 177-212) on tiny .npz files the tests write: every snapshot holds 1000 sample + time index, so
that the selection is visible in the batches.  The batches are drawn through the emulator build of the library."""
import numpy as np
import pytest

from backend_util import emu_lib

N, G, M2, TT, K = 3, 4, 2, 9, 2      # trajectories of 9 snapshots (indices 0 ... 8) on 4 x 4, corr on 2 x 2


@pytest.fixture()
def cpu():
    from fourierflow_amd import _lib
    _lib._install_test_backend(emu_lib())
    yield "cpu"
    _lib._install_test_backend(None)


def _marked(n, g, T, offset=0.0):
    """w [n, g, g, T] with w[b, ..., t] = 1000 b + t + offset."""
    return (1000.0 * np.arange(n)[:, None, None, None] + np.arange(T)[None, None, None, :] + offset + np.zeros((n, g, g, T))
            ).astype(np.float32)


@pytest.fixture(params=["vorticity", "data"])
def files(request, tmp_path):
    """The files of one split in the reference's layout (`vorticity` [n, T, X, Y] with `time`) or the generator's (`data`
    [n, X, Y, T]); the initial condition is marked 1000 b - 1, the corr trajectory 1000 b + t + 0.5."""
    w, corr = _marked(N, G, TT), _marked(N, M2, TT, 0.5)
    time = 0.25 * np.arange(1, TT + 1)
    if request.param == "vorticity":
        np.savez(tmp_path / "traj_4.npz", vorticity=np.moveaxis(w, -1, 1), time=time)
        np.savez(tmp_path / "traj_2.npz", vorticity=np.moveaxis(corr, -1, 1), time=time)
    else:
        np.savez(tmp_path / "traj_4.npz", data=w, time=time)
        np.savez(tmp_path / "traj_2.npz", data=corr)
    np.savez(tmp_path / "init_4.npz", vorticity=w[..., 0] - 1.0)
    return tmp_path, w, corr, time


def _builder(root, ext=".nc", end=None, batch_size=2, k=K):
    from fourierflow_amd.builders import KolmogorovBuilder, KolmogorovTorchDataset, KolmogorovTrajectoryDataset
    held = dict(init_path=str(root / f"init_4{ext}"), path=str(root / f"traj_4{ext}"), corr_path=str(root / f"traj_2{ext}"), k=k,
                end=end, in_memory=True)
    return KolmogorovBuilder(KolmogorovTorchDataset(str(root / f"traj_4{ext}"), k), KolmogorovTrajectoryDataset(**held),
                             KolmogorovTrajectoryDataset(**held), batch_size=batch_size, num_workers=4, pin_memory=True)


def test_training_pairs_are_the_datasets_formula(files, cpu):
    root, w, _, _ = files
    ds = _builder(root, batch_size=5).train_data(cpu, shuffle=False)
    P = TT - K                                                          # t = 0 ... T - k - 1
    assert ds.n_pairs == N * P and ds.mode == "kolmogorov" and ds.k == K
    batches = list(ds.epoch())
    assert all(set(b) == {"x", "y"} for b in batches)
    x, y = (np.concatenate([b[k].numpy() for b in batches]) for k in ("x", "y"))
    assert x.shape == y.shape == (N * P, G, G, 1)                       # the short last batch is kept
    for idx in range(N * P):
        b, t = idx // P, idx % P
        assert np.array_equal(x[idx, ..., 0], w[b, ..., t]) and np.array_equal(y[idx, ..., 0], w[b, ..., t + K])
    shuffled = _builder(root, batch_size=5).train_data(cpu, seed=3)
    first = np.concatenate([b["x"].numpy() for b in shuffled.epoch()])[:, 0, 0, 0]
    assert sorted(first) == sorted(x[:, 0, 0, 0]) and not np.array_equal(first, x[:, 0, 0, 0])


@pytest.mark.parametrize("end", [None, 7, 4])
def test_held_out_columns_follow_the_index_formulas(files, cpu, end):
    root, w, corr, time = files
    bld = _builder(root, end=end)
    for split in ("valid_data", "test_data"):
        batches = list(getattr(bld, split)(cpu).epoch())
        assert [len(b["data"]) for b in batches] == [2, 1]               # file order, the short last batch kept
        data = np.concatenate([b["data"].numpy() for b in batches])
        cd = np.concatenate([b["corr_data"].numpy() for b in batches])
        times = np.concatenate([b["times"].numpy() for b in batches])
        full = np.concatenate([w[..., :1] - 1.0, w], axis=-1)            # the initial condition in front
        assert np.array_equal(data, full[..., slice(None, end, K)])
        assert np.array_equal(cd, corr[..., slice(None, end, K)])        # no initial condition in front of corr_data
        assert np.array_equal(times, np.tile(np.concatenate([[0.0], time])[slice(None, end, K)].astype(np.float32), (N, 1)))
        # the index formulas, spelled out: column 0 is the initial condition, column j + 1 snapshot k (j + 1) - 1; corr column j
        # is snapshot k j -- ONE snapshot later than the data column it is compared with
        L, Lc = data.shape[-1], cd.shape[-1]
        assert L == len(range(0, TT + 1 if end is None else min(end, TT + 1), K))
        assert Lc == len(range(0, TT if end is None else min(end, TT), K))
        for b in range(N):
            assert data[b, 0, 0, 0] == 1000 * b - 1
            for j in range(L - 1):
                assert data[b, 0, 0, j + 1] == 1000 * b + K * (j + 1) - 1
            for j in range(Lc):
                assert cd[b, 0, 0, j] == 1000 * b + K * j + 0.5
            for j in range(1, min(L, Lc)):
                assert cd[b, 0, 0, j] - data[b, 0, 0, j] == 1.5          # 0.5 is the corr marker: the snapshot index is 1 ahead


def test_inference_data_is_the_joined_test_set_at_every_kth_time(files, cpu):
    root, w, _, _ = files
    got = _builder(root, end=4).inference_data(cpu)                       # (`end` is not applied here, as in the reference)
    assert set(got) == {"data"}
    assert np.array_equal(got["data"].numpy(), np.concatenate([w[..., :1] - 1.0, w], axis=-1)[..., ::K])


def test_default_time_and_generator_times(tmp_path, cpu):
    from fourierflow_amd.builders.kolmogorov import load_trajectories
    w = _marked(N, G, TT)
    np.savez(tmp_path / "a.npz", data=w)
    np.savez(tmp_path / "b.npz", data=w, times=np.tile(0.5 * np.arange(1, TT + 1), (N, 1)))
    assert np.array_equal(load_trajectories(str(tmp_path / "a.nc"))[1], np.arange(1, TT + 1))
    assert np.array_equal(load_trajectories(str(tmp_path / "b.npz"))[1], 0.5 * np.arange(1, TT + 1))


def test_nc_paths_map_to_npz_siblings_and_npz_paths_are_taken_as_they_are(files, cpu, monkeypatch):
    from fourierflow_amd.builders.kolmogorov import npz_path
    root, w, _, _ = files
    assert npz_path("/d/train_64_4.nc") == "/d/train_64_4.npz" and npz_path("/d/x.npz") == "/d/x.npz"
    monkeypatch.setenv("DATA_ROOT", str(root))
    assert npz_path("${DATA_ROOT}/a.nc") == str(root / "a.npz")
    a = next(_builder(root, ".nc").valid_data(cpu).epoch())
    b = next(_builder(root, ".npz").valid_data(cpu).epoch())
    assert all(np.array_equal(a[k].numpy(), b[k].numpy()) for k in ("data", "corr_data", "times"))


def test_datasets_are_light_until_used(tmp_path):
    from fourierflow_amd.builders import KolmogorovBuilder, KolmogorovTorchDataset, KolmogorovTrajectoryDataset
    held = KolmogorovTrajectoryDataset(str(tmp_path / "i.nc"), str(tmp_path / "p.nc"), str(tmp_path / "c.nc"), 20, end=None)
    bld = KolmogorovBuilder(KolmogorovTorchDataset(str(tmp_path / "t.nc"), 20, in_memory=True), held, held, batch_size=32)
    assert (bld.batch_size, bld.train_dataset.k, held.k, held.end) == (32, 20, 20, None)      # nothing was opened
    with pytest.raises(TypeError, match="train_dataset must be a KolmogorovTorchDataset"):
        KolmogorovBuilder(held, held, held)


def test_file_problems_carry_the_one_message(files, cpu):
    from fourierflow_amd.builders.kolmogorov import load_initial, load_trajectories
    root, w, _, _ = files
    common = ("`vorticity` [n, T, X, Y] or `data` [n, X, Y, T]", "`vorticity` [n, X, Y]", "xarray.open_dataset",
              "generate navier-stokes")
    with pytest.raises(FileNotFoundError) as e:
        _builder(root / "nowhere").train_data(cpu)
    assert all(word in str(e.value) for word in (*common, str(root / "nowhere" / "traj_4.npz"), "netCDF is not read"))
    np.savez(root / "empty.npz", other=np.zeros(3))
    with pytest.raises(ValueError) as e:
        load_trajectories(str(root / "empty.nc"))
    assert all(word in str(e.value) for word in (*common, "no array `vorticity` or `data`", "['other']"))
    with pytest.raises(ValueError) as e:
        load_initial(str(root / "empty.npz"))
    assert all(word in str(e.value) for word in (*common, "no array `vorticity`", "['other']"))
    with pytest.raises(ValueError) as e:
        load_initial(str(root / "traj_4.npz"))                            # a trajectory file where an initial condition belongs
    assert all(word in str(e.value) for word in (*common, "[n, X, Y], got")) or "no array `vorticity`" in str(e.value)
    np.savez(root / "short.npz", data=w, time=np.arange(3))
    with pytest.raises(ValueError) as e:
        load_trajectories(str(root / "short.npz"))
    assert all(word in str(e.value) for word in (*common, "`time` holds 3 entries"))


@pytest.mark.parametrize("name", ["KolmogorovMultiTorchDataset", "KolmogorovJAXDataset", "KolmogorovJAXTrajectoryDataset"])
def test_unsupported_datasets_are_refused_by_name(name):
    from fourierflow_amd.config import instantiate
    with pytest.raises(NotImplementedError, match=f"fourierflow.builders.{name} is not built"):
        instantiate({"_target_": f"fourierflow.builders.{name}", "path": "x.nc", "k": 4})


def test_learned_interpolator_routine_is_refused_by_name():
    from fourierflow_amd.config import build_routine
    with pytest.raises(NotImplementedError, match="fourierflow.routines.LearnedInterpolator"):
        build_routine({"routine": {"_target_": "fourierflow.routines.LearnedInterpolator", "size": 32,
                                   "optimizer": {"_target_": "optax.adamw", "weight_decay": 1e-4}}})


def test_the_builder_section_of_a_shipped_config_instantiates(tmp_path, monkeypatch):
    """experiments/torus_kochkov/ffno/ablation/ffno-nw/64/config.yaml as shipped (tests/golden/reference_configs.npz)."""
    from test_config import shipped_configs

    from fourierflow_amd.builders import KolmogorovBuilder
    from fourierflow_amd.config import instantiate, load_config
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()["torus_kochkov/ffno/ablation/ffno-nw/64/config.yaml"])
    bld = instantiate(load_config(str(cfg))["builder"])
    assert isinstance(bld, KolmogorovBuilder) and bld.batch_size == 32 and bld.train_dataset.k == bld.valid_dataset.k == 20
    assert bld.valid_dataset.corr_path == str(tmp_path / "kolmogorov/re_1000/trajectories/valid_32_4.nc")
