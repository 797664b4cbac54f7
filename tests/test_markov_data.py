"""MarkovTrajectoryData (fourierflow_amd/builders/markov_data.py): epochs of Markov pairs drawn on the device from whole
trajectories, against the numpy restatement of the reference's datasets in tests/test_kernels_markov_pairs.py and the
DataLoader rules of builders/ns_markov.py:36-41 (shuffle, drop_last=False).  Runs on the emulator and on the GPU."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from backend_util import host_device  # noqa: F401
from test_kernels_markov_pairs import kolmogorov_item, ns_markov_dataset

N_TRAJ, M, N, T, B = 4, 6, 5, 6, 3           # 4 x (6 - 2) = 16 pairs: five full batches and a short one of 1


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(31)
    data = (rs.standard_normal((N_TRAJ, M, N, T)) + 0.3).astype(np.float32)
    f = rs.standard_normal((N_TRAJ, M, N)).astype(np.float32)
    mu = rs.uniform(1e-5, 1e-3, N_TRAJ).astype(np.float32)
    full = ns_markov_dataset(data)
    for a in (data, f, mu, *full.values()):
        a.setflags(write=False)
    return data, f, mu, full


def _make(case, device, **kw):
    from fourierflow_amd.builders.markov_data import MarkovTrajectoryData
    data, f, mu, _ = case
    kw = dict(dict(device=device, batch_size=B, seed=5), **kw)
    return MarkovTrajectoryData(data, f, mu, **kw)


def _host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _pair_ids(batches, full):
    """The pair id of every yielded sample, found by matching its `x` against the expanded set (whose rows are distinct)."""
    flat = full["x"].reshape(len(full["x"]), -1)
    ids = []
    for b in batches:
        for row in b["x"].reshape(len(b["x"]), -1):
            hit = np.nonzero((flat == row).all(axis=1))[0]
            assert len(hit) == 1
            ids.append(int(hit[0]))
    return ids


def test_unshuffled_epoch_is_the_dataset_in_order(case, host_device):
    data, f, mu, full = case
    ds = _make(case, host_device, shuffle=False)
    assert ds.n_pairs == 16 and len(ds) == 6
    batches = [_host(b) for b in ds.epoch()]
    assert [len(b["x"]) for b in batches] == [3, 3, 3, 3, 3, 1]
    for j, b in enumerate(batches):
        ids = np.arange(j * B, min((j + 1) * B, 16))
        assert set(b) == {"x", "y", "dx", "dy", "f", "mu"} and b["x"].shape == (len(ids), M, N, 1)
        for name in ("x", "y", "dx", "dy"):
            assert_array_equal(b[name], full[name][ids], err_msg=name)
        assert_array_equal(b["f"], f[ids // (T - 2)])
        assert_array_equal(b["mu"], mu[ids // (T - 2)])
    again = [_host(b) for b in ds.epoch()]                    # every unshuffled epoch is the same
    assert all(a["x"].tobytes() == b["x"].tobytes() for a, b in zip(batches, again))


def test_kolmogorov_mode_with_stride(case, host_device):
    data = case[0]
    k = 2
    ds = _make(case, host_device, shuffle=False, mode="kolmogorov", k=k, batch_size=5)
    assert ds.n_pairs == N_TRAJ * (T - k) and len(ds) == 4
    got = [_host(b) for b in ds.epoch()]
    assert all(set(b) == {"x", "y", "f", "mu"} for b in got)
    for name in ("x", "y"):
        want = np.stack([kolmogorov_item(data, k, i)[name] for i in range(ds.n_pairs)])
        assert_array_equal(np.concatenate([b[name] for b in got]), want)


def test_ns_markov_mode_with_stride(case, host_device):
    """k = 2: inputs t = 2 ... T - 3, targets t + 2, dx against t - 2."""
    data = case[0]
    ds = _make(case, host_device, shuffle=False, k=2, batch_size=8)
    assert ds.n_pairs == N_TRAJ * (T - 4)
    b = _host(next(iter(ds.epoch())))
    x, y, px = (np.moveaxis(data[..., s], -1, 1).reshape(-1, M, N, 1) for s in (slice(2, T - 2), slice(4, T), slice(0, T - 4)))
    assert_array_equal(b["x"], x)
    assert_array_equal(b["y"], y)
    assert_array_equal(b["dx"], x - px)
    assert_array_equal(b["dy"], y - x)


def test_shuffled_epochs_are_seeded_permutations(case, host_device):
    _, f, mu, full = case
    ds = _make(case, host_device)
    first = [_host(b) for b in ds.epoch()]
    second = [_host(b) for b in ds.epoch()]
    ids1, ids2 = _pair_ids(first, full), _pair_ids(second, full)
    assert sorted(ids1) == list(range(16)) and sorted(ids2) == list(range(16))          # every pair exactly once
    assert ids1 != ids2 and ids1 != list(range(16))
    gen = torch.Generator().manual_seed(5)                                              # consecutive draws of one CPU generator
    assert ids1 == torch.randperm(16, generator=gen).tolist() and ids2 == torch.randperm(16, generator=gen).tolist()
    for b, lo in zip(first, range(0, 16, B)):                                           # the whole sample follows its id
        ids = np.asarray(ids1[lo:lo + B])
        for name in ("y", "dx", "dy"):
            assert_array_equal(b[name], full[name][ids])
        assert_array_equal(b["f"], f[ids // (T - 2)])
        assert_array_equal(b["mu"], mu[ids // (T - 2)])
    other = _make(case, host_device)                                                    # the same seed: the same run
    it = iter(other)                                                                    # (__iter__ chains epochs)
    replay = [_host(next(it)) for _ in range(12)]
    assert _pair_ids(replay, full) == ids1 + ids2
    assert _pair_ids([_host(b) for b in _make(case, host_device, seed=6).epoch()], full) != ids1


def test_drop_last(case, host_device):
    _, _, _, full = case
    keep, drop = _make(case, host_device), _make(case, host_device, drop_last=True)
    assert len(keep) == 6 and len(drop) == 5
    assert [len(b["x"]) for b in keep.epoch()] == [3, 3, 3, 3, 3, 1]
    dropped = [_host(b) for b in drop.epoch()]
    assert [len(b["x"]) for b in dropped] == [3] * 5
    assert len(set(_pair_ids(dropped, full))) == 15


def test_two_ranks_share_one_permutation(case, host_device):
    _, _, _, full = case
    ranks = [_make(case, host_device, batch_size=2, drop_last=True, rank=r, world=2) for r in (0, 1)]   # 8 batches: 4 each
    odd = [_make(case, host_device, rank=r, world=2) for r in (0, 1)]                   # 6 batches of 3, 3, 3, 3, 3, 1: 3 each
    five = [_make(case, host_device, drop_last=True, rank=r, world=2) for r in (0, 1)]  # 5 batches: the fifth is dropped
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(16, generator=gen).tolist()
    for pair, n_each, bs, covered in ((ranks, 4, 2, 16), (odd, 3, 3, 16), (five, 2, 3, 12)):
        got = [_pair_ids([_host(b) for b in ds.epoch()], full) for ds in pair]
        assert len(pair[0]) == len(pair[1]) == n_each
        assert not set(got[0]) & set(got[1])                                            # disjoint
        assert sorted(got[0] + got[1]) == sorted(perm[:covered])                        # all but the dropped tail
        for r in (0, 1):                                                                # rank r: batches r, r + 2, ...
            want = [i for j in range(r, 2 * n_each, 2) for i in perm[j * bs:(j + 1) * bs]]
            assert got[r] == want


def test_constructor_refusals(case, host_device):
    from fourierflow_amd import _lib
    from fourierflow_amd.builders.markov_data import MarkovTrajectoryData
    data, f, mu, _ = case
    kw = dict(device=host_device, batch_size=B, seed=0)
    with pytest.raises(ValueError, match="at least 3 steps"):
        MarkovTrajectoryData(data[..., :2], **kw)
    with pytest.raises(ValueError, match="at least 7 steps"):
        MarkovTrajectoryData(data, k=3, **kw)
    with pytest.raises(ValueError, match="at least 7 steps"):
        MarkovTrajectoryData(data, mode="kolmogorov", k=6, **kw)
    MarkovTrajectoryData(data, mode="kolmogorov", k=5, **kw)
    with pytest.raises(ValueError, match="one force map per trajectory"):
        MarkovTrajectoryData(data, f[:3], **kw)
    with pytest.raises(ValueError, match="one viscosity per trajectory"):
        MarkovTrajectoryData(data, None, mu[:2], **kw)
    with pytest.raises(ValueError, match="trajectories \\[n, M, N, T\\]"):
        MarkovTrajectoryData(data[0], **kw)
    with pytest.raises(ValueError, match="mode must be"):
        MarkovTrajectoryData(data, mode="rollout", **kw)
    with pytest.raises(ValueError, match="not one for each of 2 ranks"):
        MarkovTrajectoryData(data, **dict(kw, batch_size=16), world=2)
    other = "cuda:0" if host_device == "cpu" else "cpu"                                  # CPU data with the HIP library, and the reverse
    with pytest.raises(_lib.FFNOLibraryError, match="no CPU path"):
        MarkovTrajectoryData(data, **dict(kw, device=other))
