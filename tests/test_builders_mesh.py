"""StructuredMesh2DBuilder, PlasticityBuilder, ElasticityBuilder (fourierflow_amd/builders/mesh_data.py) on files of 12 samples the
test writes itself: split membership and order against the reference's slices restated in numpy (the cited lines), the batch
dicts the routines take, `DATA_ROOT` through the config loader.  Runs on the emulator and on the GPU."""
import numpy as np
import pytest
import scipy.io
from numpy.testing import assert_array_equal

from backend_util import host_device  # noqa: F401

N_FILE, TRAIN, VALID, TEST, B = 12, 5, 3, 2, 2
SIZES = dict(train_size=TRAIN, valid_size=VALID, test_size=TEST)


def _epoch(data):
    """Every batch of one epoch, concatenated per key, and the batch lengths."""
    batches = [{k: v.cpu().numpy() for k, v in b.items()} for b in data.epoch()]
    return {k: np.concatenate([b[k] for b in batches]) for k in batches[0]}, [len(next(iter(b.values()))) for b in batches]


def _check_splits(bld, device, want, lengths):
    """want: {split: {key: array}} -- unshuffled, the splits come out whole and in file order."""
    for split, make in (("train", lambda: bld.train_data(device, shuffle=False)), ("valid", lambda: bld.valid_data(device)),
                        ("test", lambda: bld.test_data(device))):
        got, lens = _epoch(make())
        assert lens == lengths[split], split
        assert set(got) == set(want[split])
        for k, w in want[split].items():
            assert got[k].dtype == np.float32 and got[k].shape == w.shape, (split, k, got[k].shape, w.shape)
            assert_array_equal(got[k], w, err_msg=f"{split} {k}")


LENGTHS = dict(train=[2, 2, 1], valid=[2, 1], test=[2])


# ---- airfoil / pipe ---------------------------------------------------------------------------------------------
@pytest.fixture()
def airfoil(tmp_path):
    rs = np.random.RandomState(61)
    X, Y, C = 7, 5, 3
    x1, x2, q = rs.standard_normal((N_FILE, X, Y)), rs.standard_normal((N_FILE, X, Y)), rs.standard_normal((N_FILE, C, X, Y))
    root = tmp_path / "geo-fno" / "airfoil"
    root.mkdir(parents=True)
    for name, a in (("X", x1), ("Y", x2), ("Q", q)):      # float64 files, like the dataset's
        np.save(root / f"{name}.npy", a)
    paths = dict(x1_path=str(root / "X.npy"), x2_path=str(root / "Y.npy"), sigma_path=str(root / "Q.npy"))
    return paths, x1, x2, q


def test_structured_mesh_2d_builder(airfoil, host_device):
    from fourierflow_amd.builders import StructuredMesh2DBuilder
    paths, x1, x2, q = airfoil
    bld = StructuredMesh2DBuilder(**paths, output_dim=2, **SIZES, batch_size=B, num_workers=1, pin_memory=True)
    # structured_mesh_2d.py:23-36: x = stack([x1, x2], -1), y = sigma[:, output_dim], as float
    x, y = np.stack([x1, x2], -1).astype(np.float32), q[:, 2].astype(np.float32)
    # structured_mesh_2d.py:40-46: train x[:i], TEST x[i:j], valid x[j:k]
    i, j, k = TRAIN, TRAIN + TEST, TRAIN + TEST + VALID
    want = {s: dict(x=x[sl], y=y[sl][..., None]) for s, sl in (("train", slice(0, i)), ("test", slice(i, j)), ("valid", slice(j, k)))}
    assert want["train"]["x"].shape == (5, 7, 5, 2) and want["valid"]["y"].shape == (3, 7, 5, 1)
    _check_splits(bld, host_device, want, LENGTHS)


def test_shuffled_training_epochs_follow_the_seed(airfoil, host_device):
    import torch
    from fourierflow_amd.builders import StructuredMesh2DBuilder
    paths, x1, _, _ = airfoil
    bld = StructuredMesh2DBuilder(**paths, output_dim=0, **SIZES, batch_size=B)
    data = bld.train_data(host_device, seed=3)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        got, lens = _epoch(data)
        assert lens == [2, 2, 1]
        assert_array_equal(got["x"][..., 0], x1[:TRAIN].astype(np.float32)[torch.randperm(TRAIN, generator=gen).numpy()])
    ranks = [bld.train_data(host_device, seed=3, rank=r, world=2) for r in (0, 1)]      # 3 batches: one each, the third dropped
    assert len(ranks[0]) == len(ranks[1]) == 1


# ---- plasticity --------------------------------------------------------------------------------------------------
def test_plasticity_builder(tmp_path, host_device):
    from fourierflow_amd.builders import PlasticityBuilder
    rs = np.random.RandomState(62)
    s1, s2, t = 6, 3, 2
    inp, out = rs.standard_normal((N_FILE, s1)), rs.standard_normal((N_FILE, s1, s2, t, 4))
    path = tmp_path / "plas.mat"
    scipy.io.savemat(path, dict(input=inp, output=out))
    bld = PlasticityBuilder(str(path), **SIZES, s1=s1, s2=s2, t=t, batch_size=B, num_workers=1, pin_memory=True)
    # plasticity.py:26-33: x = repeat(input, 'b s1 -> b s1 s2 t 1'), y = output, as float32
    x = np.broadcast_to(inp.astype(np.float32)[:, :, None, None, None], (N_FILE, s1, s2, t, 1))
    y = out.astype(np.float32)
    # plasticity.py:35-41: train [:i], valid [i:j], test [j:k]
    i, j, k = TRAIN, TRAIN + VALID, TRAIN + VALID + TEST
    want = {s: dict(x=x[sl], y=y[sl]) for s, sl in (("train", slice(0, i)), ("valid", slice(i, j)), ("test", slice(j, k)))}
    assert want["test"]["x"].shape == (2, 6, 3, 2, 1) and want["test"]["y"].shape == (2, 6, 3, 2, 4)
    _check_splits(bld, host_device, want, LENGTHS)


# ---- elasticity --------------------------------------------------------------------------------------------------
@pytest.fixture()
def elasticity(tmp_path):
    rs = np.random.RandomState(63)
    P = 9
    rr, sigma, xy = rs.standard_normal((42, N_FILE)), rs.standard_normal((P, N_FILE)), rs.uniform(0, 1, (P, 2, N_FILE))
    for name, a in (("rr", rr), ("sigma", sigma), ("xy", xy)):
        np.save(tmp_path / f"{name}.npy", a)
    paths = dict(sigma_path=str(tmp_path / "sigma.npy"), xy_path=str(tmp_path / "xy.npy"), rr_path=str(tmp_path / "rr.npy"))
    return paths, rr, sigma, xy


def test_elasticity_builder(elasticity, host_device):
    from fourierflow_amd.builders import ElasticityBuilder
    paths, rr, sigma, xy = elasticity
    bld = ElasticityBuilder(**paths, **SIZES, batch_size=B, num_workers=1, pin_memory=True)
    # elasticity.py:23-36: rr.permute(1, 0), sigma.permute(1, 0).unsqueeze(-1), xy.permute(2, 0, 1), as float
    full = dict(rr=rr.T.astype(np.float32), sigma=sigma.T.astype(np.float32)[..., None],
                xy=np.transpose(xy, (2, 0, 1)).astype(np.float32))
    # elasticity.py:38-49: train [:train_size], valid [-eval_size:-test_size], test [-test_size:]
    ev = VALID + TEST
    want = {s: {k: v[sl] for k, v in full.items()}
            for s, sl in (("train", slice(0, TRAIN)), ("valid", slice(-ev, -TEST)), ("test", slice(-TEST, None)))}
    assert want["valid"]["xy"].shape == (3, 9, 2) and want["valid"]["rr"].shape == (3, 42) and want["valid"]["sigma"].shape == (3, 9, 1)
    _check_splits(bld, host_device, want, LENGTHS)


# ---- config, errors ----------------------------------------------------------------------------------------------
def test_data_root_resolves_through_the_config_loader(airfoil, tmp_path, host_device, monkeypatch):
    from fourierflow_amd.builders import StructuredMesh2DBuilder
    from fourierflow_amd.config import instantiate, load_config
    _, x1, _, _ = airfoil
    cfg = tmp_path / "config.yaml"
    cfg.write_text("""
builder:
  _target_: fourierflow.builders.StructuredMesh2DBuilder
  x1_path: ${oc.env:DATA_ROOT}/geo-fno/airfoil/X.npy
  x2_path: ${oc.env:DATA_ROOT}/geo-fno/airfoil/Y.npy
  sigma_path: ${oc.env:DATA_ROOT}/geo-fno/airfoil/Q.npy
  output_dim: 1
  train_size: 5
  valid_size: 3
  test_size: 2
  batch_size: 4
  num_workers: 1
  pin_memory: true
""")
    monkeypatch.setenv("DATA_ROOT", str(tmp_path))
    bld = instantiate(load_config(str(cfg), ["builder.batch_size=5"])["builder"])
    assert type(bld) is StructuredMesh2DBuilder and bld.batch_size == 5
    got, lens = _epoch(bld.train_data(host_device, shuffle=False))
    assert lens == [5]
    assert_array_equal(got["x"][..., 0], x1[:5].astype(np.float32))


def test_missing_files_and_oversized_splits(airfoil, elasticity, tmp_path):
    from fourierflow_amd.builders import ElasticityBuilder, PlasticityBuilder, StructuredMesh2DBuilder
    paths, *_ = airfoil
    gone = str(tmp_path / "nowhere" / "Q.npy")
    with pytest.raises(FileNotFoundError, match="nowhere"):
        StructuredMesh2DBuilder(**dict(paths, sigma_path=gone), output_dim=0, **SIZES)
    with pytest.raises(FileNotFoundError, match="nowhere"):
        PlasticityBuilder(gone, **SIZES, s1=6, s2=3, t=2)
    with pytest.raises(FileNotFoundError, match="nowhere"):
        ElasticityBuilder(**dict(elasticity[0], xy_path=gone), **SIZES)
    with pytest.raises(ValueError, match=r"(?s)13.*12"):                                   # 8 + 3 + 2 = 13 of 12
        StructuredMesh2DBuilder(**paths, output_dim=0, train_size=8, valid_size=3, test_size=2)
    StructuredMesh2DBuilder(**paths, output_dim=0, train_size=7, valid_size=3, test_size=2)   # exactly the file
    with pytest.raises(ValueError, match=r"(?s)13.*12"):
        ElasticityBuilder(**elasticity[0], train_size=13, valid_size=0, test_size=0)
    with pytest.raises(ValueError, match=r"(?s)14.*12"):                                   # valid + test reach before the file's start
        ElasticityBuilder(**elasticity[0], train_size=1, valid_size=7, test_size=6)
    with pytest.raises(ValueError, match="output_dim"):
        StructuredMesh2DBuilder(**paths, output_dim=3, **SIZES)
