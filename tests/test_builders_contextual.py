"""NSContextualBuilder (fourierflow_amd/builders/ns_contextual.py) against what the reference's own datasets return
(builders/ns_contextual.py:45-101, recorded in tests/golden/contextual_ref.npz by tools/make_golden_contextual.py): every batch
of an unshuffled and of a shuffled epoch, the valid / test batches with their `times`, both force layouts (one map per
trajectory, one per snapshot), sharding over ranks, the ways `data_path` may name the files, and the refusals.  The batches are
copies: every comparison is bit for bit.  Files the tests write themselves from the fixture.  Emulator and GPU."""
import os

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from backend_util import host_device  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contextual_ref.npz")
B, SEED = 4, 5                                           # 3 x (7 - 2) = 15 pairs: three batches of 4 and one of 3
LAYOUTS = ("const", "step")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    assert g["u"].shape == (3, 8, 8, 7) and g["f_const"].shape == (3, 8, 8) and g["f_step"].shape == (3, 8, 8, 7)
    assert int(g["ssr"]) == 2 and int(g["k"]) == 2 and g["step.train.x"].shape == (15, 4, 4, 1)
    return g


@pytest.fixture(scope="module")
def files(golden, tmp_path_factory):
    """{layout: prefix}: the same set as all three splits of each prefix, at the file's full 8 x 8 (the builder strides by ssr)."""
    root = tmp_path_factory.mktemp("contextual")
    out = {}
    for layout in LAYOUTS:
        prefix = str(root / f"torus_{layout}")
        for split in ("train", "valid", "test"):
            np.savez(f"{prefix}.{split}.npz", data=golden["u"], f=golden[f"f_{layout}"], mu=golden["mu"],
                     times=np.zeros((3, 7), np.float32))
        out[layout] = prefix
    return out


def _builder(prefix, golden, **kw):
    from fourierflow_amd.builders import NSContextualBuilder
    return NSContextualBuilder(prefix, int(golden["ssr"]), int(golden["k"]), **{"batch_size": B, "num_workers": 16, "pin_memory": True, **kw})


def _host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _train_want(golden, layout):
    return {k: golden[f"{layout}.train.{k}"] for k in ("x", "y", "f", "mu")}


def _eval_want(golden, layout):
    want = {k: golden[f"{layout}.eval.{k}"] for k in ("data", "f", "mu")}
    assert golden[f"{layout}.eval.times"].dtype == np.float64         # the reference's arange; the batches carry it as float32
    want["times"] = golden[f"{layout}.eval.times"].astype(np.float32)
    return want


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unshuffled_training_batches_are_the_dataset_in_order(files, golden, host_device, layout):
    ds = _builder(files[layout], golden).train_data(host_device, seed=SEED, shuffle=False)
    want = _train_want(golden, layout)
    assert len(ds) == 4 and ds.n_pairs == 15 and ds.mode == "kolmogorov" and ds.k == 2
    batches = [_host(b) for b in ds.epoch()]
    assert [len(b["x"]) for b in batches] == [4, 4, 4, 3]
    for k in want:
        assert all(b[k].dtype == np.float32 for b in batches) and set(batches[0]) == set(want)
        assert_array_equal(np.concatenate([b[k] for b in batches]), want[k], err_msg=k)
    if layout == "step":      # the force of the target time: another map for every pair of a trajectory
        assert not np.array_equal(want["f"][0], want["f"][1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shuffled_epochs_are_seeded_permutations(files, golden, host_device, layout):
    ds = _builder(files[layout], golden).train_data(host_device, seed=SEED)
    want = _train_want(golden, layout)
    gen = torch.Generator().manual_seed(SEED)
    perms = [torch.randperm(15, generator=gen).numpy() for _ in range(2)]      # consecutive draws of one CPU generator
    assert not np.array_equal(perms[0], np.arange(15)) and not np.array_equal(perms[0], perms[1])
    for ids in perms:
        batches = [_host(b) for b in ds.epoch()]
        assert [len(b["x"]) for b in batches] == [4, 4, 4, 3]
        for k in want:
            assert_array_equal(np.concatenate([b[k] for b in batches]), want[k][ids], err_msg=k)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("split", ["valid_data", "test_data"])
def test_valid_and_test_batches(files, golden, host_device, layout, split):
    ds = getattr(_builder(files[layout], golden, batch_size=2), split)(host_device)
    want = _eval_want(golden, layout)
    assert ds.n == 3 and not ds.shuffle and len(ds) == 2
    assert want["data"].shape == (3, 4, 4, 4) and want["times"].shape == (3, 100)
    batches = [_host(b) for b in ds.epoch()]
    assert [len(b["data"]) for b in batches] == [2, 1]                 # file order, the short last batch kept
    for k in want:
        assert set(batches[0]) == set(want) and all(b[k].dtype == np.float32 for b in batches)
        assert_array_equal(np.concatenate([b[k] for b in batches]), want[k], err_msg=k)


def test_ranks_take_alternate_batches_of_one_permutation(files, golden, host_device):
    """The rule of MarkovTrajectoryData: every rank draws the SAME permutation, rank r takes batches r, r + world, ..., and the
    trailing batches that do not fill every rank are dropped (15 pairs in batches of 2: eight batches, six for three ranks)."""
    bld = _builder(files["step"], golden, batch_size=2)
    want = _train_want(golden, "step")
    perm = torch.randperm(15, generator=torch.Generator().manual_seed(SEED)).numpy()
    for rank in range(3):
        ds = bld.train_data(host_device, seed=SEED, rank=rank, world=3)
        assert len(ds) == 2
        batches = [_host(b) for b in ds.epoch()]
        for j, b in zip((rank, rank + 3), batches):
            for k in want:
                assert_array_equal(b[k], want[k][perm[2 * j:2 * j + 2]], err_msg=f"{k} of batch {j} on rank {rank}")


def test_f_and_mu_go_along_only_where_the_routine_appends_them(files, golden, host_device):
    bld = _builder(files["step"], golden)
    bld.append_force, bld.append_mu = False, True
    assert set(next(bld.train_data(host_device, shuffle=False).epoch())) == {"x", "y", "mu"}
    assert set(next(bld.valid_data(host_device).epoch())) == {"data", "mu", "times"}
    bld.append_force, bld.append_mu = True, False
    assert set(next(bld.train_data(host_device, shuffle=False).epoch())) == {"x", "y", "f"}
    assert set(next(bld.test_data(host_device).epoch())) == {"data", "f", "times"}


def test_one_upload_and_one_launch_per_batch(files, golden, host_device, monkeypatch):
    from fourierflow_amd import _capi
    from fourierflow_amd.builders import markov_data, sample_data
    uploads, launches = [], []
    real_upload, real_check = markov_data.upload, _capi.check

    def upload(t, device):
        uploads.append(t.numel())
        return real_upload(t, device)

    def check(rc, what):
        launches.append(what)
        return real_check(rc, what)

    for mod in (markov_data, sample_data):
        monkeypatch.setattr(mod, "upload", upload)
    monkeypatch.setattr(_capi, "check", check)
    bld = _builder(files["step"], golden)
    field = 3 * 4 * 4 * 7                                             # u after ssr = 2, and the per-step force
    ds = bld.train_data(host_device, seed=SEED)
    assert sorted(uploads) == [3, field, field]                       # mu, u and f once each, in the layout of the file
    for _ in range(2):
        for _ in ds.epoch():
            pass
    assert len(uploads) == 3 and launches == ["markov_pairs"] * 8
    del uploads[:], launches[:]
    held = bld.valid_data(host_device)                                # the k-stride is the gather's: u and f go up at full rate
    assert sorted(uploads) == [3, 100, field, field]
    assert len(list(held.epoch())) == 1 and launches == ["sample_gather"]


def test_markov_trajectory_data_takes_a_force_per_snapshot(golden, host_device):
    from fourierflow_amd.builders import MarkovTrajectoryData
    u, f, mu = golden["u"][:, ::2, ::2], golden["f_step"][:, ::2, ::2], golden["mu"]
    kw = dict(device=host_device, batch_size=15, seed=0, shuffle=False)
    (b,) = [_host(b) for b in MarkovTrajectoryData(u, f, mu, mode="kolmogorov", k=2, **kw).epoch()]
    assert b["f"].shape == (15, 4, 4)                                 # what _build_features takes, as with one map per trajectory
    assert_array_equal(b["f"], golden["step.train.f"])
    # ns_markov mode, k = 1: inputs 1 ... T - 2 with dx / dy; the force is still the target's, f[b, ..., t + 1]
    (b,) = [_host(b) for b in MarkovTrajectoryData(u, f, mu, mode="ns_markov", k=1, **kw).epoch()]
    assert set(b) == {"x", "y", "dx", "dy", "f", "mu"}
    assert_array_equal(b["f"], np.moveaxis(f[..., 2:], -1, 1).reshape(15, 4, 4))
    assert_array_equal(b["x"][..., 0], np.moveaxis(u[..., 1:-1], -1, 1).reshape(15, 4, 4))
    for bad in (f[..., :6], f[..., :1], f[:2], f[None], np.concatenate([f, f], axis=-1)):      # Tf = T, or no time axis
        with pytest.raises(ValueError, match="one force map per trajectory .* or one per snapshot"):
            MarkovTrajectoryData(u, bad, mu, mode="kolmogorov", k=2, **kw)


def test_data_path_names_the_prefix_any_of_the_files_or_the_h5_name(files, golden, host_device):
    prefix = files["const"]
    want = _train_want(golden, "const")
    for path in (prefix, prefix + ".train.npz", prefix + ".valid.npz", prefix + ".test.npz", prefix + ".h5"):
        bld = _builder(path, golden, batch_size=15)
        assert bld.files == {s: f"{prefix}.{s}.npz" for s in ("train", "valid", "test")}
        (b,) = [_host(b) for b in bld.train_data(host_device, shuffle=False).epoch()]
        assert_array_equal(b["y"], want["y"])


def test_environment_variables_in_the_path_and_u_as_the_key(golden, host_device, tmp_path, monkeypatch):
    for split in ("train", "valid", "test"):
        np.savez(tmp_path / f"t.{split}.npz", u=golden["u"], f=golden["f_const"], mu=golden["mu"])
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    (b,) = [_host(b) for b in _builder("$DATA_ROOT/t.h5", golden, batch_size=3).test_data(host_device).epoch()]
    assert_array_equal(b["data"], golden["const.eval.data"])


def test_refusals_carry_the_one_message(files, golden, tmp_path):
    from fourierflow_amd.builders import NSContextualBuilder
    u, f, mu = golden["u"], golden["f_const"], golden["mu"]

    def refused(path, exc, *words):
        with pytest.raises(exc) as e:
            NSContextualBuilder(path, 2, 2, batch_size=B)
        text = str(e.value)
        prefix = str(tmp_path / "p")
        for word in (*words, f"{prefix}.train.npz", f"{prefix}.valid.npz", f"{prefix}.test.npz", "`data` or `u` [n, X, Y, T]",
                     "`f` [n, X, Y] or [n, X, Y, T]", "`mu` [n]", f"generate navier-stokes {prefix} --train-trajectories --force random",
                     "--mu-min", "--mu-max"):
            assert word in text, (word, text)

    refused(str(tmp_path / "p"), FileNotFoundError, "not found")                           # none of the three
    refused(str(tmp_path / "p.h5"), FileNotFoundError, "HDF5", "siblings")                 # the reference's own file name alone
    (tmp_path / "p.h5").write_bytes(b"\x89HDF\r\n\x1a\n")
    refused(str(tmp_path / "p.h5"), FileNotFoundError, "HDF5", "siblings")                 # ... even where that file exists
    np.savez(tmp_path / "p.train.npz", data=u, f=f, mu=mu)
    np.savez(tmp_path / "p.valid.npz", data=u, f=f, mu=mu)
    refused(str(tmp_path / "p.train.npz"), FileNotFoundError, "not found", "p.test.npz")   # one of the three missing
    for absent, named in (("mu", "`mu`"), ("f", "`f`"), ("data", "`data` or `u`")):
        arrays = dict(data=u, f=f, mu=mu)
        del arrays[absent]
        np.savez(tmp_path / "p.test.npz", **arrays)
        refused(str(tmp_path / "p"), ValueError, f"p.test.npz: no array {named}")
    np.savez(tmp_path / "p.test.npz", data=u, f=f, mu=mu)
    NSContextualBuilder(str(tmp_path / "p"), 2, 2)
    with pytest.raises(ValueError, match="at least 1"):
        NSContextualBuilder(str(tmp_path / "p"), 0, 2)
    with pytest.raises(ValueError, match="at least 1"):
        NSContextualBuilder(str(tmp_path / "p"), 2, 0)
    with pytest.raises(ValueError, match=r"T = 7 steps.* at least 8"):
        NSContextualBuilder(str(tmp_path / "p"), 2, 7).arrays("train")
    np.savez(tmp_path / "p.test.npz", data=u, f=f[:, :4], mu=mu)
    with pytest.raises(ValueError, match=r"expected data \[n, X, Y, T\], f \[n, X, Y\] or \[n, X, Y, T\]"):
        NSContextualBuilder(str(tmp_path / "p"), 2, 2).arrays("test")
