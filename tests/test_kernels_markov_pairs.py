"""ffno_markov_pairs (include/ffno.h) through the C ABI against a numpy restatement of the reference's two pair datasets,
NavierStokesTrainingDataset (builders/ns_markov.py:62-91) and KolmogorovTorchDataset (builders/kolmogorov.py:125-139), on the
emulator and on the GPU.  Every output is a copy or one fp32 subtraction of two fp32 values, which numpy rounds the same way:
the comparisons are `assert_array_equal`, no tolerance."""
import itertools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from backend_util import be  # noqa: F401

OUTPUTS = ("x", "y", "dx", "dy", "f", "mu")


def ns_markov_dataset(data):
    """NavierStokesTrainingDataset.__init__ (ns_markov.py:62-80): `rearrange(., 'b m n t -> (b t) m n 1')` is a transpose + reshape."""
    def expand(a):
        return np.ascontiguousarray(np.moveaxis(a, -1, 1)).reshape(-1, a.shape[1], a.shape[2], 1)

    return dict(x=expand(data[..., 1:-1]), y=expand(data[..., 2:]), dx=expand(data[..., 1:-1] - data[..., :-2]),
                dy=expand(data[..., 2:] - data[..., 1:-1]))


def kolmogorov_item(data, k, idx):
    """KolmogorovTorchDataset.__getitem__ (kolmogorov.py:125-139): `isel(time=slice(t, t + k + 1, k))`, first and second entry."""
    T = data.shape[-1] - k
    b, t = idx // T, idx % T
    pair = data[b][..., t:t + k + 1:k]
    return dict(x=pair[..., 0:1], y=pair[..., 1:2])


def _case(seed, n, M, N, T):
    rs = np.random.RandomState(seed)
    return ((rs.standard_normal((n, M, N, T)) + 0.3).astype(np.float32), rs.standard_normal((n, M, N)).astype(np.float32),
            rs.uniform(1e-5, 1e-3, n).astype(np.float32))


def _call(be, data, ids, outs, t0, k, P, f=None, mu=None):
    """One launch writing the outputs named in `outs` into NaN-prefilled arrays -> (rc, {name: array} for ALL six names)."""
    lib, p = be.lib, be.ptr
    n, M, N, T = data.shape
    B = len(ids)
    shapes = dict(x=(B, M, N, 1), y=(B, M, N, 1), dx=(B, M, N, 1), dy=(B, M, N, 1), f=(B, M, N), mu=(B,))
    d = {name: be.empty(shapes[name]) for name in OUTPUTS}
    arg = {name: p(d[name]) if name in outs else None for name in OUTPUTS}
    rc = lib.ffno_markov_pairs(p(be.put(data)), p(be.put(np.asarray(ids, np.int32))), arg["x"], arg["y"], arg["dx"], arg["dy"],
                               p(be.put(f)), arg["f"], p(be.put(mu)), arg["mu"], n, M, N, T, t0, k, P, B, None)
    return rc, {name: be.get(d[name]) for name in OUTPUTS}


def _check(got, want, outs):
    for name in OUTPUTS:
        if name in outs:
            assert_array_equal(got[name], want[name], err_msg=name)
        else:
            assert np.isnan(got[name]).all(), f"{name} was not requested and must keep its prefill"


def _ns_want(data, f, mu, ids):
    ids = np.asarray(ids)
    T = data.shape[-1]
    want = {k: v[ids] for k, v in ns_markov_dataset(data).items()}
    want.update(f=f[ids // (T - 2)], mu=mu[ids // (T - 2)])
    return want


@pytest.mark.parametrize("shape,ids", [
    ((3, 5, 7, 3), [2, 0, 1, 0]),                        # one pair per trajectory, odd sizes
    ((4, 8, 12, 6), [0, 3, 15, 12, 3]),                  # first and last pair of a trajectory (0, 3; 12, 15), a repeated id
    ((2, 64, 64, 20), [35, 0, 17]),                      # the real row length
])
def test_ns_markov_pairs_equal_the_dataset(be, shape, ids):
    data, f, mu = _case(21, *shape)
    T = shape[-1]
    rc, got = _call(be, data, ids, OUTPUTS, 1, 1, T - 2, f, mu)
    assert rc == 0
    _check(got, _ns_want(data, f, mu, ids), OUTPUTS)


def test_kolmogorov_pairs_equal_the_dataset(be):
    n, M, N, T, k = 3, 6, 4, 7, 2
    data, f, mu = _case(22, n, M, N, T)
    ids = [0, 14, 4, 5]                                   # T - k = 5 pairs per trajectory: first, last, and both sides of a boundary
    outs = ("x", "y", "f", "mu")
    rc, got = _call(be, data, ids, outs, 0, k, T - k, f, mu)
    assert rc == 0
    items = [kolmogorov_item(data, k, i) for i in ids]
    b = np.asarray(ids) // (T - k)
    _check(got, dict(x=np.stack([it["x"] for it in items]), y=np.stack([it["y"] for it in items]), f=f[b], mu=mu[b]), outs)


SUBSETS = [s for r in range(1, 7) for s in itertools.combinations(OUTPUTS, r) if set(s) & {"x", "y", "dx", "dy"}]


def test_every_subset_of_outputs(be):
    """60 subsets (every one with at least one field output), one tiny launch each: what is not requested keeps its NaN prefill."""
    data, f, mu = _case(23, 4, 8, 12, 6)
    ids = [0, 3, 15, 12, 3]
    want = _ns_want(data, f, mu, ids)
    assert len(SUBSETS) == 60
    for outs in SUBSETS:
        rc, got = _call(be, data, ids, outs, 1, 1, 4, f, mu)
        assert rc == 0, outs
        _check(got, want, outs)


def test_bad_ids_give_nan_samples_and_nothing_else(be):
    n, M, N, T = 4, 8, 12, 6
    data, f, mu = _case(24, n, M, N, T)
    P = T - 2
    ids = [5, n * P, 9, -1, 0]
    rc, got = _call(be, data, ids, OUTPUTS, 1, 1, P, f, mu)
    assert rc == 0
    good = [0, 2, 4]
    want = _ns_want(data, f, mu, [ids[i] for i in good])
    for name in OUTPUTS:
        assert np.isnan(got[name][[1, 3]]).all(), name
        assert_array_equal(got[name][good], want[name], err_msg=name)


def test_host_rejections(be):
    lib, p = be.lib, be.ptr
    a, ids = be.zeros((4096,)), be.put(np.zeros(4, np.int32))
    A, I = p(a), p(ids)

    def call(data=A, ids=I, x=A, y=None, dx=None, dy=None, f=None, f_out=None, mu=None, mu_out=None, n=2, M=4, N=4, T=6, t0=1,
             k=1, P=4, B=4):
        return lib.ffno_markov_pairs(data, ids, x, y, dx, dy, f, f_out, mu, mu_out, n, M, N, T, t0, k, P, B, None)

    assert call() == 0
    assert call(dx=A, f=A, f_out=A, mu=A, mu_out=A) == 0
    assert call(data=None) == -1 and call(ids=None) == -1
    assert call(x=None) == -1                                  # none of x, y, dx, dy
    for size in ("n", "M", "N", "T", "k", "P", "B"):
        assert call(**{size: 0}) == -1 and call(**{size: -1}) == -1, size
    assert call(t0=-1) == -1
    assert call(t0=1, P=5) == -1                                # t0 + P - 1 + k = 6 > T - 1
    assert call(t0=0, P=5) == 0                                 # ... = 5: the last pair ends on the last step
    assert call(t0=0, k=2, P=5) == -1
    assert call(t0=0, P=4, dx=A) == -1                          # dx reads t - k
    assert call(t0=2, k=2, P=2, dx=A) == 0
    assert call(f_out=A) == -1 and call(mu_out=A) == -1         # gathers without their source


def test_two_calls_are_bit_identical(be):
    data, f, mu = _case(25, 2, 64, 64, 20)
    ids = [35, 0, 17]
    _, a = _call(be, data, ids, OUTPUTS, 1, 1, 18, f, mu)
    _, b = _call(be, data, ids, OUTPUTS, 1, 1, 18, f, mu)
    for name in OUTPUTS:
        assert a[name].tobytes() == b[name].tobytes(), name
