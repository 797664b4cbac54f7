"""ffno_markov_pairs_tf (include/ffno.h) through the C ABI against numpy indexing: the pairs of the contextual
NavierStokesTrainingDataset (builders/ns_contextual.py:45-72), whose force is one map per trajectory or one per snapshot --
then the map of the pair's TARGET time, f[b, ..., t + k].  On the emulator and on the GPU.  Every output is a copy or one fp32
subtraction of two fp32 values, which numpy rounds the same way: the comparisons are `assert_array_equal`, no tolerance.

Shapes: the smallest that can go wrong.  n = 3 trajectories of M x N = 5 x 6 (unequal axes; 30 pixels, no multiple of 4) and of
4 x 8, T = 7; B = 5 ids holding the first and the last pair of the set, a repeated id and one id = n P, whose sample must be NaN
in every requested output while the others stay correct.  Every output buffer carries guard words behind it."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from backend_util import be  # noqa: F401

OUTPUTS = ("x", "y", "dx", "dy", "f", "mu")
GUARD, SENTINEL = 8, np.float32(12345.0)
n, T = 3, 7


def _case(seed, M, N, Tf):
    rs = np.random.RandomState(seed)
    data = (rs.standard_normal((n, M, N, T)) + 0.3).astype(np.float32)
    f = rs.standard_normal((n, M, N, Tf) if Tf else (n, M, N)).astype(np.float32)
    return data, f, rs.uniform(1e-5, 1e-3, n).astype(np.float32)


def _want(data, f, mu, Tf, ids, t0, k, P):
    """{name: [B, ...]} by plain indexing; an id outside [0, n P) gives a NaN sample."""
    _, M, N, _ = data.shape
    out = dict(x=[], y=[], dx=[], dy=[], f=[], mu=[])
    for p in ids:
        if not 0 <= p < n * P:
            for name in ("x", "y", "dx", "dy"):
                out[name].append(np.full((M, N, 1), np.nan, np.float32))
            out["f"].append(np.full((M, N), np.nan, np.float32))
            out["mu"].append(np.float32(np.nan))
            continue
        b, t = p // P, t0 + p % P
        x, y = data[b, :, :, t:t + 1], data[b, :, :, t + k:t + k + 1]
        out["x"].append(x)
        out["y"].append(y)
        out["dx"].append(x - data[b, :, :, t - k:t - k + 1] if t >= k else np.full((M, N, 1), np.nan, np.float32))
        out["dy"].append(y - x)
        out["f"].append(f[b, :, :, t + k] if Tf else f[b])
        out["mu"].append(mu[b])
    return {name: np.stack(v) for name, v in out.items()}


def _shapes(B, M, N):
    return dict(x=(B, M, N, 1), y=(B, M, N, 1), dx=(B, M, N, 1), dy=(B, M, N, 1), f=(B, M, N), mu=(B,))


def _call(be, data, f, mu, Tf, ids, outs, t0, k, P, entry="ffno_markov_pairs_tf"):
    """One launch writing the outputs named in `outs` -> (rc, {name: array}, {name: guard words}) for ALL six names; every buffer
    is prefilled with SENTINEL and is GUARD floats longer than its output."""
    lib, p = be.lib, be.ptr
    _, M, N, _ = data.shape
    B = len(ids)
    shapes = _shapes(B, M, N)
    bufs = {name: be.put(np.full(int(np.prod(shapes[name])) + GUARD, SENTINEL, np.float32)) for name in OUTPUTS}
    arg = {name: p(bufs[name]) if name in outs else None for name in OUTPUTS}
    head = (p(be.put(data)), p(be.put(np.asarray(ids, np.int32))), arg["x"], arg["y"], arg["dx"], arg["dy"], p(be.put(f)))
    tail = (arg["f"], p(be.put(mu)), arg["mu"], n, M, N, T, t0, k, P, B, None)
    if entry == "ffno_markov_pairs_tf":
        rc = lib.ffno_markov_pairs_tf(*head, Tf, *tail)
    else:
        rc = lib.ffno_markov_pairs(*head, *tail)
    flat = {name: np.asarray(be.get(bufs[name])) for name in OUTPUTS}
    return rc, {name: flat[name][:-GUARD].reshape(shapes[name]) for name in OUTPUTS}, {name: flat[name][-GUARD:] for name in OUTPUTS}


def _check(got, guards, want, outs):
    for name in OUTPUTS:
        assert (guards[name] == SENTINEL).all(), f"the guard words behind {name} were written"
        if name in outs:
            assert_array_equal(got[name], want[name], err_msg=name)
        else:
            assert (got[name] == SENTINEL).all(), f"{name} was not requested and must keep its prefill"


# (t0, k, P, outputs, ids): the contextual dataset's pairs, t0 = 0 and P = T - k; and a window with room for dx.  ids: the first
# and the last pair of the set, a repeated id, and n P -- one past the last
KOLMOGOROV = (0, 2, 5, ("x", "y", "f", "mu"), [0, 14, 7, 7, 15])
WITH_DX = (2, 2, 3, OUTPUTS, [0, 8, 4, 4, 9])


@pytest.mark.parametrize("M,N", [(5, 6), (4, 8)])
@pytest.mark.parametrize("t0,k,P,outs,ids", [KOLMOGOROV, WITH_DX])
def test_per_step_force_equals_indexing(be, M, N, t0, k, P, outs, ids):
    data, f, mu = _case(31, M, N, T)
    rc, got, guards = _call(be, data, f, mu, T, ids, outs, t0, k, P)
    assert rc == 0
    want = _want(data, f, mu, T, ids, t0, k, P)
    bad = [i for i, p in enumerate(ids) if p >= n * P]
    assert len(bad) == 1 and all(np.isnan(want[name][bad]).all() for name in outs)
    assert not any(np.isnan(want[name][:bad[0]]).any() for name in outs)
    _check(got, guards, want, outs)
    # the force at the target time, not at the input's: they differ in this set
    good = [i for i in range(len(ids)) if i not in bad]
    at_input = np.stack([f[ids[i] // P, :, :, t0 + ids[i] % P] for i in good])
    assert not np.array_equal(got["f"][good], at_input)


def test_force_rows_longer_than_the_trajectories(be):
    """Tf is f's own row length: a force array with more maps than snapshots is read with ITS stride."""
    t0, k, P, outs, ids = KOLMOGOROV
    data, f, mu = _case(32, 5, 6, T + 2)
    rc, got, guards = _call(be, data, f, mu, T + 2, ids, outs, t0, k, P)
    assert rc == 0
    _check(got, guards, _want(data, f, mu, T + 2, ids, t0, k, P), outs)


@pytest.mark.parametrize("t0,k,P,outs,ids", [KOLMOGOROV, WITH_DX])
def test_constant_force_is_ffno_markov_pairs(be, t0, k, P, outs, ids):
    """Tf = 0: one map per trajectory -- the old entry's outputs, bit for bit, and numpy's."""
    data, f, mu = _case(33, 5, 6, 0)
    rc_new, new, guards_new = _call(be, data, f, mu, 0, ids, outs, t0, k, P)
    rc_old, old, guards_old = _call(be, data, f, mu, 0, ids, outs, t0, k, P, entry="ffno_markov_pairs")
    assert rc_new == 0 and rc_old == 0
    for name in OUTPUTS:
        assert new[name].tobytes() == old[name].tobytes(), name
    want = _want(data, f, mu, 0, ids, t0, k, P)
    _check(new, guards_new, want, outs)
    _check(old, guards_old, want, outs)


@pytest.mark.parametrize("outs", [("x",), ("y", "f"), ("dy", "f"), ("dx", "mu"), ("x", "y", "dx", "dy", "mu"), ("y", "f", "mu")])
def test_optional_outputs_may_be_null(be, outs):
    t0, k, P, _, ids = WITH_DX
    data, f, mu = _case(34, 5, 6, T)
    rc, got, guards = _call(be, data, f, mu, T, ids, outs, t0, k, P)
    assert rc == 0
    _check(got, guards, _want(data, f, mu, T, ids, t0, k, P), outs)


def test_host_rejections_launch_nothing(be):
    lib, p = be.lib, be.ptr
    a, ids = be.zeros((4096,)), be.put(np.zeros(4, np.int32))
    A, I = p(a), p(ids)
    outputs = {name: be.put(np.full(4 * 4 * 4 + GUARD, SENTINEL, np.float32)) for name in ("x", "f_out")}

    def call(data=A, ids=I, x=p(outputs["x"]), y=None, dx=None, dy=None, f=A, Tf=6, f_out=p(outputs["f_out"]), mu=None, mu_out=None,
             n=2, M=4, N=4, T=6, t0=1, k=1, P=4, B=4):
        return lib.ffno_markov_pairs_tf(data, ids, x, y, dx, dy, f, Tf, f_out, mu, mu_out, n, M, N, T, t0, k, P, B, None)

    def untouched():
        return all((np.asarray(be.get(t)) == SENTINEL).all() for t in outputs.values())

    # the new cases: a negative Tf, and force rows that end before the last pair's target (t0 + P - 1 + k = 5 > Tf - 1)
    assert call(Tf=-1) == -1 and call(Tf=-6) == -1
    assert call(Tf=5) == -1 and call(Tf=1) == -1
    assert call(t0=0, k=2, P=4, Tf=5) == -1                     # T = 6 holds the pair, f's 5 maps do not
    # ... and those of ffno_markov_pairs, unchanged under a per-step force
    assert call(data=None) == -1 and call(ids=None) == -1
    assert call(x=None) == -1                                  # none of x, y, dx, dy
    for size in ("n", "M", "N", "T", "k", "P", "B"):
        assert call(**{size: 0}) == -1 and call(**{size: -1}) == -1, size
    assert call(t0=-1) == -1
    assert call(t0=1, P=5) == -1                                # t0 + P - 1 + k = 6 > T - 1
    assert call(t0=0, P=4, dx=A) == -1                          # dx reads t - k
    assert call(f=None) == -1 and call(mu_out=A) == -1          # gathers without their source
    assert call(f=None, Tf=0) == -1
    assert untouched()                                          # none of them launched
    # the boundaries that ARE valid
    assert call() == 0                                          # t0 + P - 1 + k = 5 = Tf - 1: the last pair's force is f's last map
    assert call(Tf=7) == 0 and call(Tf=0) == 0
    assert call(t0=0, P=5, Tf=6) == 0
    assert call(f=None, f_out=None, Tf=6) == 0                  # no force asked for
    assert not untouched()
