"""KolmogorovMultiResolutionDataset / MultiResolutionMarkovData (fourierflow_amd/builders/kolmogorov.py, markov_data.py): the
training set of the torus_kochkov/ffno/multi_resolution configs -- the reference's KolmogorovMultiTorchDataset
(builders/kolmogorov.py:142-174) under DataLoader(shuffle=True, num_workers=W), restated here in plain Python and simulated worker by
worker.  Marked files: snapshot t of trajectory b of set s holds 1000 b + t + s / 4 everywhere, so that a batch shows which set and
which (b, t) it was drawn from.  The batches are drawn through the emulator build of the library, and on the GPU."""
import numpy as np
import pytest
import torch

from backend_util import emu_lib, host_device  # noqa: F401

MULTI = "fourierflow_amd.builders.KolmogorovMultiResolutionDataset"
CONFIGS = ["x32_x64", "x32_x128", "x64_x128"]


@pytest.fixture()
def cpu():
    from fourierflow_amd import _lib
    _lib._install_test_backend(emu_lib())
    yield "cpu"
    _lib._install_test_backend(None)


# ---- the reference's dataset and loader, restated -------------------------------------------------------------------------------
class _ReferenceDataset:
    """KolmogorovMultiTorchDataset: `counter` and `ds_index`, advanced by every item (builders/kolmogorov.py:148-174)."""

    def __init__(self, n_sets, B, T, batch_size):
        self.n_sets, self.B, self.T, self.batch_size = n_sets, B, T, batch_size
        self.counter, self.ds_index = 0, 0

    def __getitem__(self, idx):
        item = (self.ds_index, idx // self.T, idx % self.T)      # (file, b, t)
        self.counter += 1
        if self.counter % self.batch_size == 0:
            self.ds_index = (self.ds_index + 1) % self.n_sets
        return item


def _reference_epoch(order, n_sets, B, T, batch_size, W):
    """The batches of one epoch of DataLoader(dataset, batch_size, num_workers=W) over the sampler's `order`: every worker holds
    its own copy of the dataset (counter at zero: the copy is made when the epoch's iterator starts), batch j goes to worker
    j % W."""
    workers = [_ReferenceDataset(n_sets, B, T, batch_size) for _ in range(W)]
    batches = [order[lo:lo + batch_size] for lo in range(0, len(order), batch_size)]
    return [[workers[j % W][int(idx)] for idx in batch] for j, batch in enumerate(batches)]


def _marked(n, g, T, s):
    return (1000.0 * np.arange(n)[:, None, None, None] + np.arange(T)[None, None, None, :] + 0.25 * s + np.zeros((n, g, g, T))
            ).astype(np.float32)


def _decode(batch, k):
    """[(set, b, t)] of a batch of marked data; y must be the same pair k later."""
    x, y = batch["x"].cpu().numpy(), batch["y"].cpu().numpy()
    assert set(batch) == {"x", "y"} and x.shape == y.shape and x.shape[-1] == 1
    assert np.array_equal(x, np.broadcast_to(x[:, :1, :1], x.shape)) and np.array_equal(y, x + k)
    v = x[:, 0, 0, 0].astype(np.float64)
    return [(int(round(4 * (a % 1))), int(a) // 1000, int(a) % 1000) for a in v]


def _set(n_sets, n, T, k, bs, W, device, **kw):
    from fourierflow_amd.builders import MultiResolutionMarkovData
    arrays = [_marked(n, 2 * (s + 1), T, s) for s in range(n_sets)]      # grids 2, 4, 6
    return MultiResolutionMarkovData(arrays, device=device, batch_size=bs, k=k, num_workers=W, seed=kw.pop("seed", 5), **kw)


@pytest.mark.parametrize("bs", [2, 3], ids=["multiple", "short_last"])      # 20 pairs: 10 batches of 2 / 6 of 3 and one of 2
@pytest.mark.parametrize("n_sets", [2, 3])
@pytest.mark.parametrize("W", [0, 1, 2, 4])
def test_schedule_is_the_loaders(cpu, W, n_sets, bs):
    n, T, k = 4, 7, 2
    P = T - k
    data = _set(n_sets, n, T, k, bs, W, cpu)
    assert data.n_pairs == n * P and len(data) == -(-n * P // bs) and data.sizes == [(2 * (s + 1),) * 2 for s in range(n_sets)]
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        order = torch.randperm(n * P, generator=gen).tolist()
        want = _reference_epoch(order, n_sets, n, P, bs, max(1, W))      # (num_workers = 0 behaves as one worker)
        got = [_decode(b, k) for b in data.epoch()]
        assert all(len({s for s, _, _ in batch}) == 1 for batch in want)      # every batch is single-set in the reference ...
        assert got == want                                                     # ... and here: the same set, the same pairs
        assert got[0][0][0] == 0                                               # every epoch starts again at set 0
        assert [batch[0][0] for batch in got] == [(i // max(1, W)) % n_sets for i in range(len(got))]
        assert [data.set_index(i) for i in range(len(got))] == [batch[0][0] for batch in got]


def test_unshuffled_and_drop_last(cpu):
    data = _set(2, 4, 7, 2, 3, 1, cpu, shuffle=False, drop_last=True)
    got = [_decode(b, 2) for b in data.epoch()]
    assert len(got) == len(data) == 6 and got == _reference_epoch(list(range(20)), 2, 4, 5, 3, 1)[:6]
    assert [_decode(b, 2) for b in data.epoch()] == got


@pytest.mark.parametrize("W", [1, 2])
def test_ranks_step_the_same_size_together(cpu, W):
    n, T, k, bs = 4, 7, 2, 3                                                    # 7 batches: 3 per rank, the seventh dropped
    ranks = [_set(2, n, T, k, bs, W, cpu, rank=r, world=2) for r in range(2)]
    order = torch.randperm(n * (T - k), generator=torch.Generator().manual_seed(5)).tolist()
    steps = list(zip(*(r.epoch() for r in ranks)))
    assert len(steps) == len(ranks[0]) == len(ranks[1]) == 3
    for i, step in enumerate(steps):
        a, b = (_decode(batch, k) for batch in step)
        assert {s for s, _, _ in a} == {s for s, _, _ in b} == {(i // W) % 2}      # the rank's own batch position decides
        for r, got in enumerate((a, b)):                                            # rank r takes batches r, r + 2, ...
            j = r + 2 * i
            assert [(p // (T - k), p % (T - k)) for p in order[j * bs:(j + 1) * bs]] == [(bb, t) for _, bb, t in got]


@pytest.mark.parametrize("e", [1, 2])
def test_skip_epochs_gives_the_next_epoch_of_a_fresh_set(cpu, e):
    fresh, resumed = _set(3, 4, 7, 2, 3, 2, cpu), _set(3, 4, 7, 2, 3, 2, cpu)
    epochs = [[_decode(b, 2) for b in fresh.epoch()] for _ in range(e + 1)]
    resumed.skip_epochs(e)
    assert [_decode(b, 2) for b in resumed.epoch()] == epochs[e] and epochs[e] != epochs[0]
    assert epochs[e][0][0][0] == 0


# ---- batches: the reference's items, exactly ------------------------------------------------------------------------------------
def _files(root, sizes, n, T, seed=3):
    rs = np.random.RandomState(seed)
    ws = [rs.standard_normal((n, g, g, T)).astype(np.float32) for g in sizes]
    for i, (g, w) in enumerate(zip(sizes, ws)):
        if i % 2:
            np.savez(root / f"train_{g}_4.npz", data=w)                                      # the generator's layout
        else:
            np.savez(root / f"train_{g}_4.npz", vorticity=np.moveaxis(w, -1, 1))             # the reference's
    return ws


def _builder(root, sizes, k, bs, W, ds_bs=None, ext=".nc"):
    from fourierflow_amd.builders import KolmogorovBuilder, KolmogorovMultiResolutionDataset, KolmogorovTrajectoryDataset
    held = KolmogorovTrajectoryDataset(str(root / "i.nc"), str(root / "p.nc"), str(root / "c.nc"), k)
    ds = KolmogorovMultiResolutionDataset([str(root / f"train_{g}_4{ext}") for g in sizes], k, bs if ds_bs is None else ds_bs)
    return KolmogorovBuilder(ds, held, held, batch_size=bs, num_workers=W, pin_memory=True)


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("shuffle", [False, True])
def test_batches_are_the_scheduled_sets_pairs(tmp_path, host_device, shuffle, W):
    """n = 2, T = 6, k = 2, batches of 3: 8 pairs in batches of 3, 3 and 2 -- on grids 8 and 16 on the emulator, 32 and 64 on the GPU."""
    sizes = (8, 16) if host_device == "cpu" else (32, 64)
    n, T, k, bs = 2, 6, 2, 3
    ws = _files(tmp_path, sizes, n, T)
    bld = _builder(tmp_path, sizes, k, bs, W)
    assert len(bld.train_dataset) == n * (T - k) and bld.num_workers == W
    data = bld.train_data(host_device, seed=9, shuffle=shuffle)
    assert data.device == torch.device(host_device) or data.device.type == "cuda"
    gen = torch.Generator().manual_seed(9)
    for _ in range(2):
        order = torch.randperm(8, generator=gen).tolist() if shuffle else list(range(8))
        batches = list(data.epoch())
        assert [len(b["x"]) for b in batches] == [3, 3, 2]
        for i, batch in enumerate(batches):
            s = (i // W) % 2
            w = ws[s]
            ids = order[i * bs:(i + 1) * bs]
            assert set(batch) == {"x", "y"} and tuple(batch["x"].shape) == (len(ids), sizes[s], sizes[s], 1)
            x, y = batch["x"].cpu().numpy(), batch["y"].cpu().numpy()
            for row, p in enumerate(ids):
                b, t = p // (T - k), p % (T - k)
                assert np.array_equal(x[row, ..., 0], w[b, ..., t]) and np.array_equal(y[row, ..., 0], w[b, ..., t + k])


def test_single_file_builder_is_unchanged_and_ignores_num_workers(tmp_path, cpu):
    from fourierflow_amd.builders import KolmogorovBuilder, KolmogorovTorchDataset, KolmogorovTrajectoryDataset, MarkovTrajectoryData
    _files(tmp_path, (4,), 2, 6)
    held = KolmogorovTrajectoryDataset(str(tmp_path / "i.nc"), str(tmp_path / "p.nc"), str(tmp_path / "c.nc"), 2)
    sets = [KolmogorovBuilder(KolmogorovTorchDataset(str(tmp_path / "train_4_4.nc"), 2), held, held, batch_size=3,
                              num_workers=W).train_data(cpu, seed=1) for W in (0, 4)]
    assert all(type(s) is MarkovTrajectoryData for s in sets)
    for a, b in zip(sets[0].epoch(), sets[1].epoch()):
        assert np.array_equal(a["x"].numpy(), b["x"].numpy())


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_files_that_disagree_are_refused_with_their_names_and_numbers(tmp_path, cpu):
    from fourierflow_amd.builders import KolmogorovMultiResolutionDataset
    rs = np.random.RandomState(0)
    np.savez(tmp_path / "a.npz", data=rs.standard_normal((3, 4, 4, 6)).astype(np.float32))
    np.savez(tmp_path / "fewer.npz", data=rs.standard_normal((2, 8, 8, 6)).astype(np.float32))
    np.savez(tmp_path / "shorter.npz", data=rs.standard_normal((3, 8, 8, 5)).astype(np.float32))
    a = str(tmp_path / "a.nc")
    with pytest.raises(ValueError, match=r"fewer\.npz holds n = 2 trajectories of T = 6 snapshots, .*a\.npz n = 3 of T = 6"):
        KolmogorovMultiResolutionDataset([a, str(tmp_path / "fewer.nc")], 2, 3).arrays()
    with pytest.raises(ValueError, match=r"shorter\.npz holds n = 3 trajectories of T = 5 snapshots, .*a\.npz n = 3 of T = 6"):
        len(KolmogorovMultiResolutionDataset([a, str(tmp_path / "shorter.npz")], 2, 3))
    with pytest.raises(ValueError, match=r"a\.npz, .*a\.npz: trajectories of T = 6 snapshots, a pair k = 6 apart needs at least 7"):
        KolmogorovMultiResolutionDataset([a, a], 6, 3).arrays()
    with pytest.raises(ValueError, match="paths names at least one trajectory file, got 0"):
        KolmogorovMultiResolutionDataset([], 2, 3)
    with pytest.raises(ValueError, match="k .* is at least 1, got 0"):
        KolmogorovMultiResolutionDataset([a], 0, 3)
    with pytest.raises(FileNotFoundError, match=r"dataset file not found: .*missing\.npz.*netCDF is not read"):
        KolmogorovMultiResolutionDataset([a, str(tmp_path / "missing.nc")], 2, 3).arrays()
    ds = KolmogorovMultiResolutionDataset([a, a], 2, 3)                       # light until used; a lone path is a list of one
    assert (ds.k, ds.batch_size, len(ds)) == (2, 3, 3 * 4) and KolmogorovMultiResolutionDataset(a, 2, 3).paths == [a]


def test_builder_refuses_a_batch_size_of_its_own_and_other_datasets(tmp_path):
    from fourierflow_amd.builders import KolmogorovBuilder
    with pytest.raises(ValueError, match=r"train_dataset\.batch_size = 4 but the builder's batch_size = 3"):
        _builder(tmp_path, (8, 16), 2, 3, 4, ds_bs=4)
    ok = _builder(tmp_path, (8, 16), 2, 3, 4)                                  # nothing was opened
    with pytest.raises(TypeError, match="train_dataset must be a KolmogorovTorchDataset or a KolmogorovMultiResolutionDataset, got "
                                        "KolmogorovTrajectoryDataset"):
        KolmogorovBuilder(ok.valid_dataset, ok.valid_dataset, ok.test_dataset)
    with pytest.raises(TypeError, match="valid_dataset must be a KolmogorovTrajectoryDataset, got KolmogorovMultiResolutionDataset"):
        KolmogorovBuilder(ok.train_dataset, ok.train_dataset, ok.test_dataset)


def test_device_set_refusals(cpu):
    from fourierflow_amd.builders import MultiResolutionMarkovData
    kw = dict(device=cpu, batch_size=2, k=2, seed=0)
    with pytest.raises(ValueError, match="set 1 holds 3 trajectories of 6 snapshots, set 0 2 of 6"):
        MultiResolutionMarkovData([_marked(2, 2, 6, 0), _marked(3, 4, 6, 1)], **kw)
    with pytest.raises(ValueError, match="set 1 holds 2 trajectories of 7 snapshots, set 0 2 of 6"):
        MultiResolutionMarkovData([_marked(2, 2, 6, 0), _marked(2, 4, 7, 1)], **kw)
    with pytest.raises(ValueError, match="at least one grid size, got none"):
        MultiResolutionMarkovData([], **kw)
    with pytest.raises(ValueError, match="num_workers is at least 0, got -1"):
        MultiResolutionMarkovData([_marked(2, 2, 6, 0)], num_workers=-1, **kw)
    with pytest.raises(ValueError, match="needs trajectories of at least 3 steps"):
        MultiResolutionMarkovData([_marked(2, 2, 2, 0)], **kw)


def test_the_references_own_name_is_still_refused():
    from fourierflow_amd.config import TARGET_MAP, instantiate
    assert TARGET_MAP["fourierflow.builders.KolmogorovMultiTorchDataset"] == "fourierflow_amd.builders.KolmogorovMultiTorchDataset"
    with pytest.raises(NotImplementedError, match="fourierflow.builders.KolmogorovMultiTorchDataset is not built") as e:
        instantiate({"_target_": "fourierflow.builders.KolmogorovMultiTorchDataset", "paths": ["a.nc", "b.nc"], "k": 20,
                     "batch_size": 32})
    assert MULTI in str(e.value) and "DESIGN.md section 7" in str(e.value)      # ... and says under which name it runs


# ---- the three shipped configs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_shipped_multi_resolution_configs_build_with_the_one_override(tmp_path, monkeypatch, name):
    from test_config import shipped_configs

    from fourierflow_amd.builders import KolmogorovBuilder, KolmogorovMultiResolutionDataset
    from fourierflow_amd.config import build_routine, instantiate, load_config
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(shipped_configs()[f"torus_kochkov/ffno/multi_resolution/{name}/config.yaml"])
    with pytest.raises(NotImplementedError, match="fourierflow.builders.KolmogorovMultiTorchDataset is not built"):
        instantiate(load_config(str(cfg))["builder"])
    loaded = load_config(str(cfg), [f"builder.train_dataset._target_={MULTI}"])
    bld = instantiate(loaded["builder"])
    sizes = sorted(int(s[1:]) for s in name.split("_"))
    assert isinstance(bld, KolmogorovBuilder) and isinstance(bld.train_dataset, KolmogorovMultiResolutionDataset)
    bs = 32 if name == "x32_x64" else 8
    assert (bld.batch_size, bld.num_workers, bld.train_dataset.batch_size, bld.train_dataset.k) == (bs, 4, bs, 20)
    # (the finer grid is the first path: set 0, the one every epoch starts with)
    assert bld.train_dataset.paths == [str(tmp_path / f"kolmogorov/re_1000/trajectories/train_{g}_4.nc") for g in sizes[::-1]]
    routine = build_routine(loaded)
    assert routine.use_velocity and all(hasattr(routine, f"kx_{g}") for g in sizes)
    assert (routine.conv.width, routine.conv.modes, routine.conv.n_layers) == (64, 16, 24)
