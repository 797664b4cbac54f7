"""DeviceEpochs.skip_epochs (fourierflow_amd/builders/device_epochs.py): what `train --builder --resume` advances the permutation
stream with.  After skip_epochs(n) an epoch yields the batches of a fresh set's epoch n + 1 with the same seed; an unshuffled set
draws nothing from its generator.  Emulator and GPU."""
import numpy as np
import pytest

from backend_util import host_device  # noqa: F401

SKIP = 2


def _markov(device, **kw):
    from fourierflow_amd.builders import MarkovTrajectoryData
    data = np.random.RandomState(3).standard_normal((3, 6, 5, 7)).astype(np.float32)      # 3 x (7 - 2) = 15 pairs: 4 4 4 3
    return MarkovTrajectoryData(data, device=device, batch_size=4, mode="ns_markov", k=1, seed=11, **kw)


def _samples(device, **kw):
    from fourierflow_amd.builders import DeviceSampleData
    from fourierflow_amd.builders.sample_data import rows
    source = np.random.RandomState(4).standard_normal((7, 5)).astype(np.float32)          # 7 samples: 3 3 1
    return DeviceSampleData([rows("rows", source)], 7, device=device, batch_size=3, seed=11, **kw)


def _epoch(ds):
    return [{k: v.cpu().numpy() for k, v in b.items()} for b in ds.epoch()]


@pytest.mark.parametrize("make, sizes", [(_markov, [4, 4, 4, 3]), (_samples, [3, 3, 1])])
def test_skip_epochs_then_an_epoch_is_the_fresh_sets_next_epoch(make, sizes, host_device):
    fresh = make(host_device)
    epochs = [_epoch(fresh) for _ in range(SKIP + 1)]
    assert any(not np.array_equal(a[k], b[k]) for a, b in zip(epochs[0], epochs[SKIP]) for k in a)      # the epochs do differ
    resumed = make(host_device)
    resumed.skip_epochs(SKIP)
    got = _epoch(resumed)
    assert [len(next(iter(b.values()))) for b in got] == sizes
    for a, b in zip(got, epochs[SKIP], strict=True):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("make", [_markov, _samples])
def test_an_unshuffled_set_draws_nothing(make, host_device):
    ds = make(host_device, shuffle=False)
    before = ds.gen.get_state().clone()
    ds.skip_epochs(SKIP)
    first = _epoch(ds)
    assert ds.gen.get_state().equal(before)
    fresh = _epoch(make(host_device, shuffle=False))
    assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(first, fresh, strict=True) for k in a)
