"""DeviceSampleData (fourierflow_amd/builders/sample_data.py): epochs of batches drawn on the device from named fields, against
numpy indexing and the DataLoader rules of the reference's builders (shuffle, drop_last=False; structured_mesh_2d.py:48-53).
Runs on the emulator and on the GPU."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from backend_util import host_device  # noqa: F401

N, B = 11, 3            # three full batches and a short one of 2
SEED = 5


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(51)
    a, c = rs.standard_normal((N, 4, 3)).astype(np.float32), rs.standard_normal((N, 7)).astype(np.float32)
    a[:, 0, 0] = np.arange(N)          # the sample's id, readable from the batch
    a.setflags(write=False)
    c.setflags(write=False)
    return a, c


def _make(case, device, **kw):
    from fourierflow_amd.builders.sample_data import DeviceSampleData, Field, rows
    a, c = case
    # `a` transposed in the copy ([4, 3] -> [3, 4, 1]: a real layout change), `c` as it is
    fields = [Field("a", a, (3, 4, 1), 3, 4, (12, 0, 1, 3), (0, 4, 1)), rows("c", c)]
    return DeviceSampleData(fields, N, **dict(dict(device=device, batch_size=B, seed=SEED), **kw))


def _host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def _ids(batches):
    return [int(v) for b in batches for v in b["a"][:, 0, 0, 0]]


def _check_follow(batches, case):
    a, c = case
    for b in batches:
        ids = np.asarray(_ids([b]))
        assert set(b) == {"a", "c"} and b["a"].dtype == np.float32
        assert_array_equal(b["a"], np.transpose(a[ids], (0, 2, 1))[..., None])
        assert_array_equal(b["c"], c[ids])


def test_unshuffled_epochs_are_consecutive_slices(case, host_device):
    ds = _make(case, host_device, shuffle=False)
    assert len(ds) == 4
    for _ in range(2):                                   # every unshuffled epoch is the same
        batches = [_host(b) for b in ds.epoch()]
        assert [len(b["a"]) for b in batches] == [3, 3, 3, 2]
        assert _ids(batches) == list(range(N))
        _check_follow(batches, case)


def test_shuffled_epochs_are_seeded_permutations(case, host_device):
    ds = _make(case, host_device)
    first, second = [_host(b) for b in ds.epoch()], [_host(b) for b in ds.epoch()]
    ids1, ids2 = _ids(first), _ids(second)
    assert sorted(ids1) == list(range(N)) and sorted(ids2) == list(range(N))            # every id exactly once per epoch
    gen = torch.Generator().manual_seed(SEED)                                           # consecutive draws of one CPU generator
    assert ids1 == torch.randperm(N, generator=gen).tolist() and ids2 == torch.randperm(N, generator=gen).tolist()
    assert ids1 != ids2 and ids1 != list(range(N))
    _check_follow(first + second, case)
    it = iter(_make(case, host_device))                                                 # the same seed: the same run; __iter__ chains epochs
    assert _ids([_host(next(it)) for _ in range(8)]) == ids1 + ids2
    assert _ids([_host(b) for b in _make(case, host_device, seed=SEED + 1).epoch()]) != ids1


def test_drop_last(case, host_device):
    keep, drop = _make(case, host_device), _make(case, host_device, drop_last=True)
    assert len(keep) == 4 and len(drop) == 3
    assert [len(b["a"]) for b in keep.epoch()] == [3, 3, 3, 2]
    dropped = [_host(b) for b in drop.epoch()]
    assert [len(b["a"]) for b in dropped] == [3, 3, 3] and len(set(_ids(dropped))) == 9


def test_two_ranks_share_one_permutation(case, host_device):
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(SEED)).tolist()
    # batches of 3: 3, 3, 3, 2 -> 2 each;  drop_last: 3 batches -> 1 each, the third dropped;  batches of 2 (6: 2, 2, 2, 2, 2, 1) -> 3 each
    for kw, bs, n_each, covered in ((dict(), 3, 2, 11), (dict(drop_last=True), 3, 1, 6), (dict(batch_size=2), 2, 3, 11)):
        pair = [_make(case, host_device, rank=r, world=2, **kw) for r in (0, 1)]
        got = [_ids([_host(b) for b in ds.epoch()]) for ds in pair]
        assert len(pair[0]) == len(pair[1]) == n_each
        assert not set(got[0]) & set(got[1])                                            # disjoint
        assert sorted(got[0] + got[1]) == sorted(perm[:covered])                        # the epoch minus the dropped tail
        for r in (0, 1):                                                                # rank r: batches r, r + 2, ...
            assert got[r] == [i for j in range(r, 2 * n_each, 2) for i in perm[j * bs:(j + 1) * bs]]


def test_the_set_is_its_own_copy(host_device):
    from fourierflow_amd.builders.sample_data import DeviceSampleData, rows
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    t = torch.arange(8, dtype=torch.float32).reshape(4, 2)
    want_a, want_t = a.copy(), t.numpy().copy()
    ds = DeviceSampleData([rows("a", a), rows("t", t)], 4, device=host_device, batch_size=4, shuffle=False)
    a += 100
    t += 100
    b = _host(next(iter(ds)))
    assert_array_equal(b["a"], want_a)
    assert_array_equal(b["t"], want_t)


def test_gather_takes_ids_at_an_offset(case, host_device):
    a, c = case
    ds = _make(case, host_device)
    ids = torch.tensor([9, 9, 0, 10, 4], dtype=torch.int32).to(host_device)
    b = _host(ds.gather(ids, 1, 3))
    assert_array_equal(b["c"], c[[9, 0, 10]])
    with pytest.raises(ValueError, match="outside the 5 ids"):
        ds.gather(ids, 3, 3)
    with pytest.raises(ValueError, match="int32"):
        ds.gather(ids.long(), 0, 2)


def test_constructor_refusals(case, host_device):
    from fourierflow_amd import _lib
    from fourierflow_amd.builders.sample_data import DeviceSampleData, Field, rows
    a, c = case
    kw = dict(device=host_device, batch_size=B)
    with pytest.raises(ValueError, match="not one for each of 2 ranks"):
        DeviceSampleData([rows("c", c)], N, **dict(kw, batch_size=N), world=2)
    with pytest.raises(ValueError, match="1 to 8 fields"):
        DeviceSampleData([rows(f"c{i}", c) for i in range(9)], N, **kw)
    with pytest.raises(ValueError, match="reaches float"):                                # a source shorter than n rows
        DeviceSampleData([rows("c", c)], N + 1, **kw)
    with pytest.raises(ValueError, match="reaches float"):                                # a destination past its sample
        DeviceSampleData([Field("c", c, (7,), 1, 7, (7, 0, 0, 1), (1, 0, 1))], N, **kw)
    with pytest.raises(ValueError, match="rank 2"):
        DeviceSampleData([rows("c", c)], N, rank=2, world=2, **kw)
    other = "cuda:0" if host_device == "cpu" else "cpu"                                  # CPU data with the HIP library, and the reverse
    with pytest.raises(_lib.FFNOLibraryError, match="no CPU path"):
        DeviceSampleData([rows("c", c)], N, **dict(kw, device=other))
