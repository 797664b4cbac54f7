"""NSMarkovBuilder / NSZongyiBuilder (fourierflow_amd/builders/ns_data.py) against a restatement of the reference's datasets
(builders/ns_markov.py:12-106, ns_zongyi.py:12-86): every batch of a shuffled and of an unshuffled epoch, the valid / test split,
inference_data, the file formats and the refusals.  The batches are copies (and, for dx / dy, one fp32 subtraction that numpy
rounds the same way): every comparison is bit for bit.  Files the tests write themselves.  Emulator and GPU."""
import numpy as np
import pytest
import scipy.io
import torch
from numpy.testing import assert_array_equal

from backend_util import host_device  # noqa: F401
from test_kernels_markov_pairs import ns_markov_dataset

N, T, TRAIN, TEST, B, SEED = 7, 6, 4, 2, 3, 5            # Markov: 4 x (6 - 2) = 16 pairs: five batches of 3 and one of 1
N_STEPS = 2                                              # Zongyi: 4 samples: a batch of 3 and one of 1


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{grid: (path of the .mat file, u)} for grids 16 and 32 (the latter for ssr = 2), and the 16-grid as two .npz files."""
    root = tmp_path_factory.mktemp("ns")
    rs = np.random.RandomState(83)
    out = {}
    for G in (16, 32):
        u = (rs.standard_normal((N, G, G, T)) + 0.3).astype(np.float32)
        scipy.io.savemat(root / f"u{G}.mat", {"u": u})
        u.setflags(write=False)
        out[G] = (str(root / f"u{G}.mat"), u)
    np.savez(root / "u.npz", u=out[16][1])
    np.savez(root / "data.npz", data=out[16][1], times=np.zeros((N, T), np.float32))
    out["npz"] = (str(root / "u.npz"), str(root / "data.npz"))
    return out


def _host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _epoch_ids(n, shuffle, epochs=2):
    """The ids of consecutive epochs: file order, or consecutive draws of one CPU generator seeded with SEED."""
    gen = torch.Generator().manual_seed(SEED)
    return [torch.randperm(n, generator=gen).numpy() if shuffle else np.arange(n) for _ in range(epochs)]


def _check_epochs(ds, want, n, shuffle):
    assert len(ds) == -(-n // B)
    for ids in _epoch_ids(n, shuffle):
        batches = [_host(b) for b in ds.epoch()]
        assert [len(b[next(iter(want))]) for b in batches] == [min(B, n - lo) for lo in range(0, n, B)]
        for j, b in enumerate(batches):
            assert set(b) == set(want)
            for k in want:
                assert b[k].dtype == np.float32
                assert_array_equal(b[k], want[k][ids[j * B:(j + 1) * B]], err_msg=f"{k} of batch {j}")
    if shuffle:
        assert not np.array_equal(_epoch_ids(n, True)[0], np.arange(n))


def _zongyi_want(u, append_pos):
    """ns_zongyi.py:24-35: a, the two X-tick channels on it, and u."""
    n, X, Y, _ = u.shape
    a, y = u[..., :N_STEPS], u[..., N_STEPS:2 * N_STEPS]
    if append_pos:
        ticks = torch.linspace(0, 1, X).numpy()
        gx = np.broadcast_to(ticks[None, :, None, None], (n, X, Y, 1))
        gy = np.broadcast_to(ticks[None, None, :, None], (n, X, Y, 1))
        a = np.concatenate([a, gx, gy], axis=-1)
    return dict(x=np.ascontiguousarray(a), y=np.ascontiguousarray(y), times=np.tile(np.arange(10, 20, dtype=np.float32), (n, 1)))


@pytest.mark.parametrize("ssr", [1, 2])
@pytest.mark.parametrize("shuffle", [False, True])
def test_markov_training_batches(files, host_device, ssr, shuffle):
    from fourierflow_amd.builders import NSMarkovBuilder
    path, u = files[16 * ssr]
    bld = NSMarkovBuilder(path, TRAIN, TEST, ssr, batch_size=B, num_workers=4, pin_memory=True)
    want = ns_markov_dataset(u[:TRAIN, ::ssr, ::ssr])
    assert want["x"].shape == (TRAIN * (T - 2), 16, 16, 1)
    _check_epochs(bld.train_data(host_device, seed=SEED, shuffle=shuffle), want, TRAIN * (T - 2), shuffle)


@pytest.mark.parametrize("ssr", [1, 2])
@pytest.mark.parametrize("append_pos", [True, False])
@pytest.mark.parametrize("shuffle", [False, True])
def test_zongyi_training_batches(files, host_device, ssr, append_pos, shuffle):
    from fourierflow_amd.builders import NSZongyiBuilder
    path, u = files[16 * ssr]
    bld = NSZongyiBuilder(path, TRAIN, TEST, ssr, N_STEPS, append_pos=append_pos, batch_size=B, num_workers=4)
    want = _zongyi_want(u[:TRAIN, ::ssr, ::ssr], append_pos)
    assert want["x"].shape == (TRAIN, 16, 16, N_STEPS + 2 * append_pos)
    _check_epochs(bld.train_data(host_device, seed=SEED, shuffle=shuffle), want, TRAIN, shuffle)


@pytest.mark.parametrize("ssr", [1, 2])
def test_valid_and_test_are_the_last_trajectories_in_file_order(files, host_device, ssr):
    from fourierflow_amd.builders import NSMarkovBuilder, NSZongyiBuilder
    path, u = files[16 * ssr]
    tail = u[-TEST:, ::ssr, ::ssr]
    markov = NSMarkovBuilder(path, TRAIN, TEST, ssr, batch_size=B)
    zongyi = NSZongyiBuilder(path, TRAIN, TEST, ssr, N_STEPS, batch_size=1)
    want_m = dict(data=tail, times=np.tile(np.arange(0, 20, dtype=np.float32)[:T], (TEST, 1)))
    want_z = _zongyi_want(tail, True)
    for split in ("valid_data", "test_data"):
        ds = getattr(markov, split)(host_device)
        assert ds.n == TEST and not ds.shuffle and len(ds) == 1
        (b,) = [_host(b) for b in ds.epoch()]
        assert set(b) == {"data", "times"}
        assert_array_equal(b["data"], want_m["data"])
        assert_array_equal(b["times"], want_m["times"])
        ds = getattr(zongyi, split)(host_device)
        batches = [_host(b) for b in ds.epoch()]
        assert len(batches) == TEST
        for i, b in enumerate(batches):
            for k in want_z:
                assert_array_equal(b[k], want_z[k][i:i + 1], err_msg=k)


def test_overlapping_ranges_are_kept(files, host_device):
    """train_size + test_size > n is no error in the reference: the ranges overlap."""
    from fourierflow_amd.builders import NSMarkovBuilder
    path, u = files[16]
    bld = NSMarkovBuilder(path, N, N, 1, batch_size=N)
    (b,) = [_host(b) for b in bld.test_data(host_device).epoch()]
    assert_array_equal(b["data"], u)
    assert bld.train_data(host_device, shuffle=False).n_pairs == N * (T - 2)


def test_inference_data_ignores_ssr(files, host_device):
    from fourierflow_amd.builders import NSMarkovBuilder, NSZongyiBuilder
    path, u = files[32]
    for bld in (NSMarkovBuilder(path, TRAIN, TEST, 2, batch_size=B), NSZongyiBuilder(path, TRAIN, TEST, 2, N_STEPS),
                NSMarkovBuilder(path, TRAIN, TEST, 1)):
        got = bld.inference_data(host_device)
        assert set(got) == {"data"} and got["data"].device.type == torch.device(host_device).type
        assert_array_equal(got["data"].cpu().numpy(), u)             # min(512, 7) trajectories on the file's own 32 x 32 grid


def test_npz_files_equal_the_mat_file(files, host_device):
    from fourierflow_amd.builders import NSMarkovBuilder, NSZongyiBuilder
    mat, u = files[16]
    for path in files["npz"]:
        for cls, extra in ((NSMarkovBuilder, ()), (NSZongyiBuilder, (N_STEPS,))):
            a, b = cls(mat, TRAIN, TEST, 1, *extra, batch_size=B), cls(path, TRAIN, TEST, 1, *extra, batch_size=B)
            assert a.u.dtype == b.u.dtype == np.float32
            assert_array_equal(a.u, u)
            assert_array_equal(b.u, u)
            ba, bb = _host(next(a.train_data(host_device, seed=SEED).epoch())), _host(next(b.train_data(host_device, seed=SEED).epoch()))
            for k in ba:
                assert_array_equal(ba[k], bb[k], err_msg=k)


def test_refusals(files, tmp_path, monkeypatch):
    from fourierflow_amd.builders import NSMarkovBuilder, NSZongyiBuilder
    path, u = files[16]
    with pytest.raises(ValueError, match=r"train_size = 8 .* 1 \.\.\. 7"):
        NSMarkovBuilder(path, N + 1, TEST, 1)
    with pytest.raises(ValueError, match=r"test_size = 9 .* 1 \.\.\. 7"):
        NSZongyiBuilder(path, TRAIN, N + 2, 1, N_STEPS)
    with pytest.raises(ValueError, match=r"T = 6 steps.* at least 8"):
        NSZongyiBuilder(path, TRAIN, TEST, 1, 4)
    NSZongyiBuilder(path, TRAIN, TEST, 1, 3)                          # T = 2 n_steps fits
    np.savez(tmp_path / "short.npz", u=u[..., :2])
    with pytest.raises(ValueError, match=r"T = 2 steps.* at least 3"):
        NSMarkovBuilder(str(tmp_path / "short.npz"), TRAIN, TEST, 1)
    np.savez(tmp_path / "oblong.npz", u=u[:, :, :12])
    NSMarkovBuilder(str(tmp_path / "oblong.npz"), TRAIN, TEST, 1)      # the Markov pairs do not mind
    with pytest.raises(ValueError, match=r"square grids only.* 16 x 12"):
        NSZongyiBuilder(str(tmp_path / "oblong.npz"), TRAIN, TEST, 1, N_STEPS)
    np.savez(tmp_path / "other.npz", w=u)
    with pytest.raises(ValueError, match="no array `u` or `data`"):
        NSMarkovBuilder(str(tmp_path / "other.npz"), TRAIN, TEST, 1)
    with pytest.raises(FileNotFoundError):
        NSMarkovBuilder(str(tmp_path / "absent.mat"), TRAIN, TEST, 1)

    def v73(*a, **kw):
        raise NotImplementedError("Please use HDF reader for matlab v7.3 files, e.g. h5py")

    monkeypatch.setattr(scipy.io, "loadmat", v73)
    with pytest.raises(ValueError, match=r"HDF5.*\.npz"):
        NSMarkovBuilder(path, TRAIN, TEST, 1)


def test_one_upload_of_the_training_set_and_one_launch_per_batch(files, host_device, monkeypatch):
    from fourierflow_amd import _capi
    from fourierflow_amd.builders import NSMarkovBuilder, NSZongyiBuilder, markov_data, ns_data, sample_data
    path, u = files[16]
    uploads, launches = [], []
    real_upload, real_check = markov_data.upload, _capi.check

    def upload(t, device):
        uploads.append(t.numel())
        return real_upload(t, device)

    def check(rc, what):
        launches.append(what)
        return real_check(rc, what)

    for mod in (markov_data, sample_data, ns_data):
        monkeypatch.setattr(mod, "upload", upload)
    monkeypatch.setattr(_capi, "check", check)
    train_floats = u[:TRAIN].size
    for bld, what, n in ((NSMarkovBuilder(path, TRAIN, TEST, 1, batch_size=B), "markov_pairs", TRAIN * (T - 2)),
                         (NSZongyiBuilder(path, TRAIN, TEST, 1, N_STEPS, batch_size=B), "sample_gather", TRAIN)):
        del uploads[:], launches[:]
        ds = bld.train_data(host_device, seed=SEED)
        assert uploads.count(train_floats) == 1 and sum(uploads) < train_floats + 16 * 16 * 2 + 10 + 1      # u once; positions, times
        for _ in range(2):
            for _ in ds.epoch():
                pass
        assert uploads.count(train_floats) == 1                        # ... and never again
        assert launches == [what] * (2 * -(-n // B))
        del launches[:]
        batches = list(bld.valid_data(host_device).epoch())
        assert launches == ["sample_gather"] * len(batches) and len(batches) == 1
