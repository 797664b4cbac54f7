"""ffno_markov_traj_step / ffno_markov_traj_metrics (include/ffno.h; reference routines/grid_2d_markov.py:295-372) through
the C ABI against float64 numpy, on the emulator and on the GPU.

Bounds.  A per-sample sum adds n = M N products: a thread's fma chain of n / (256 S) terms, the butterfly of a wave, four
waves, S slices -- a pairwise tree for all but the short chain, whose error is at most (ceil(log2 n) + 3) 2^-24 of the sum of
the terms' magnitudes; at n = 65536 that is 19 * 2^-24 = 1.1e-6, and 2e-6 holds for every shape run here.  For the five sums
of non-negative terms this is a RELATIVE bound; for sum P yy the magnitudes add up to at most sqrt(sum P^2 sum yy^2)
(Cauchy-Schwarz), which scales the absolute bound.  The products themselves are formed from fp32 P, raw, y (rounded once each,
relative 2^-24 per factor, inside the same budget since the terms are compared against float64 arithmetic on those same
fp32 values).

preds / im: `raw = fma(out, std, mean)` is one fused multiply-add (as in ffno_lploss_fwd_bwd), so it may differ from the
twice-rounded `out * std + mean` by the rounding of the product, at most 1 ulp of `out * std`; the sum `prev + raw` is a
plain fp32 add.  The test therefore requires bit equality with fp32(prev + fp32(fma(out, std, mean))) and at most 1 ulp of the
product (plus a rounding of raw and of the final sum, which that ulp can flip) from the unfused order.
"""
import numpy as np
import pytest

from backend_util import be  # noqa: F401

NS = 6


def _slices(lib, B, M, N, n_steps):
    ws = int(lib.ffno_markov_traj_ws_floats(B, M, N, n_steps))
    assert ws > 0 and ws % (n_steps * B * NS) == 0
    return ws, ws // (n_steps * B * NS)


def _case(seed, B, M, N, T):
    rs = np.random.RandomState(seed)
    out = rs.standard_normal((B, M, N)).astype(np.float32)
    prev = rs.standard_normal((B, M, N)).astype(np.float32)
    data = (rs.standard_normal((B, M, N, T)) + 0.3).astype(np.float32)
    affine = np.array([1.7, -0.4], np.float32)
    return out, prev, data, affine


def _reference(out, prev, data, affine, n_steps, t):
    """float64 sums over the fp32 values the kernel holds: raw = fp32(fma), P = fp32(prev + raw), y = fp32 difference."""
    T = data.shape[-1]
    yy = data[..., T - n_steps:]
    raw = out if affine is None else (out.astype(np.float64) * np.float64(affine[0]) + np.float64(affine[1])).astype(np.float32)
    P = raw if prev is None else (prev + raw).astype(np.float32)
    yt = yy[..., t]
    y = yt if prev is None else (yt - yy[..., t - 1]).astype(np.float32)        # numpy's -1 at t = 0 == the reference's wrap
    r, P6, y6, yt6 = raw.astype(np.float64), P.astype(np.float64), y.astype(np.float64), yt.astype(np.float64)
    ax = (1, 2)
    sums = np.stack([((r - y6) ** 2).sum(ax), (y6 ** 2).sum(ax), (P6 ** 2).sum(ax), (yt6 ** 2).sum(ax), (P6 * yt6).sum(ax),
                     ((P6 - yt6) ** 2).sum(ax)], axis=-1)
    return raw, P, sums


def _run_step(be, out, prev, data, affine, n_steps, t):
    lib, p = be.lib, be.ptr
    B, M, N, T = data.shape
    ws, S = _slices(lib, B, M, N, n_steps)
    d_im, d_preds, d_sums = be.empty((B, M, N)), be.empty((B, M, N, n_steps)), be.empty((ws,))
    rc = lib.ffno_markov_traj_step(p(be.put(out)), p(be.put(affine)), p(be.put(prev)), p(be.put(data)), p(d_im), p(d_preds),
                                   p(d_sums), B, M, N, T, n_steps, t, None)
    assert rc == 0
    sums = be.get(d_sums).reshape(n_steps, B, S, NS).astype(np.float64)
    return be.get(d_im), be.get(d_preds), sums, S


def _check_sums(got, want):
    for k in (0, 1, 2, 3, 5):
        err = np.abs(got[:, k] - want[:, k]) / want[:, k]
        print(f"sum {k}: max rel err {err.max():.3e}")
        assert err.max() < 2e-6, (k, err)
    err = np.abs(got[:, 4] - want[:, 4]) / np.sqrt(want[:, 2] * want[:, 3])
    print(f"sum 4: max err / sqrt(sum P^2 sum yy^2) {err.max():.3e}")
    assert err.max() < 2e-6, err


@pytest.mark.parametrize("t", [0, 2])
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("with_affine", [False, True])
def test_traj_step_matches_float64(be, with_affine, with_prev, t):
    B, M, N, T, n_steps = 3, 12, 16, 7, 4
    out, prev, data, affine = _case(11, B, M, N, T)
    affine = affine if with_affine else None
    prev = prev if with_prev else None
    im, preds, sums, S = _run_step(be, out, prev, data, affine, n_steps, t)
    raw, P, want = _reference(out, prev, data, affine, n_steps, t)
    assert S == 1
    assert np.array_equal(im, P) and np.array_equal(preds[..., t], P)          # bit-exact in the fused order
    if with_affine:                                                              # the unfused order rounds the product first
        prod = (out * affine[0]).astype(np.float32)
        unfused = prod + affine[1] if prev is None else prev + (prod + affine[1])
        assert np.all(np.abs(im.astype(np.float64) - unfused) <= np.spacing(np.abs(prod)) + np.spacing(np.abs(raw)) + np.spacing(np.abs(P)))
    other = [k for k in range(n_steps) if k != t]
    assert np.isnan(preds[..., other]).all() and np.isnan(sums[other]).all()     # one step writes its own column only
    _check_sums(sums[t].sum(axis=1), want)


def test_traj_step_sums_several_slices_per_sample(be):
    B, M, N, T, n_steps, t = 2, 64, 64, 5, 3, 1
    out, prev, data, affine = _case(12, B, M, N, T)
    im, preds, sums, S = _run_step(be, out, prev, data, affine, n_steps, t)
    assert S == 4
    raw, P, want = _reference(out, prev, data, affine, n_steps, t)
    assert np.array_equal(im, P) and np.array_equal(preds[..., t], P)
    assert (sums[t][:, :, 1] > 0).all()                 # every slice carries its own share
    _check_sums(sums[t].sum(axis=1), want)


def test_traj_step_difference_target_at_step_zero_is_the_last_step(be):
    """yy[..., t - 1] with t = 0 is Python's index -1 in the reference (:309-310): y = yy[0] - yy[n_steps - 1]."""
    B, M, N, T, n_steps = 3, 12, 16, 7, 4
    out, prev, data, _ = _case(13, B, M, N, T)
    _, _, sums, _ = _run_step(be, out, prev, data, None, n_steps, 0)
    y_last = (data[..., T - n_steps] - data[..., T - 1]).astype(np.float64)
    y_clamped = (data[..., T - n_steps] - data[..., T - n_steps - 1]).astype(np.float64)
    got = sums[0].sum(axis=1)[:, 1]
    assert np.allclose(got, (y_last ** 2).sum((1, 2)), rtol=2e-6)
    assert not np.allclose(got, (y_clamped ** 2).sum((1, 2)), rtol=1e-3)


def test_traj_step_in_place_on_prev(be):
    """The routine keeps one buffer for `prev` and `im`."""
    lib, p = be.lib, be.ptr
    B, M, N, T, n_steps, t = 3, 12, 16, 7, 4, 1
    out, prev, data, affine = _case(14, B, M, N, T)
    ws, S = _slices(lib, B, M, N, n_steps)
    d_im, d_preds, d_sums = be.put(prev), be.empty((B, M, N, n_steps)), be.empty((ws,))
    assert lib.ffno_markov_traj_step(p(be.put(out)), p(be.put(affine)), p(d_im), p(be.put(data)), p(d_im), p(d_preds), p(d_sums),
                                     B, M, N, T, n_steps, t, None) == 0
    _, P, _ = _reference(out, prev, data, affine, n_steps, t)
    assert np.array_equal(be.get(d_im), P)


def test_traj_step_rejects_bad_arguments(be):
    lib, p = be.lib, be.ptr
    a = be.zeros((64,))
    assert lib.ffno_markov_traj_step(None, None, None, p(a), p(a), p(a), p(a), 1, 2, 2, 4, 2, 0, None) != 0
    assert lib.ffno_markov_traj_step(p(a), None, None, p(a), p(a), p(a), p(a), 1, 2, 2, 4, 5, 0, None) != 0     # n_steps > T
    assert lib.ffno_markov_traj_step(p(a), None, None, p(a), p(a), p(a), p(a), 1, 2, 2, 4, 2, 2, None) != 0     # t >= n_steps
    assert lib.ffno_markov_traj_metrics(None, p(a), 1, 2, 2, 2, 0.95, None) != 0
    assert lib.ffno_markov_traj_ws_floats(0, 2, 2, 2) == 0


def _metrics(be, sums, B, M, N, n_steps, threshold=0.95):
    lib, p = be.lib, be.ptr
    d_m = be.empty((4 + 2 * n_steps,))
    assert lib.ffno_markov_traj_metrics(p(be.put(sums.astype(np.float32))), p(d_m), B, M, N, n_steps, threshold, None) == 0
    return be.get(d_m).astype(np.float64)


def _hand_sums(p_target, B, S, rs):
    """sums[t][b][slice][6] whose correlation s4 / (sqrt(s2) sqrt(s3)) is p_target[t] for every sample, spread over S slices."""
    n_steps = len(p_target)
    tot = np.zeros((n_steps, B, NS))
    tot[..., 0] = rs.uniform(1, 2, (n_steps, B))
    tot[..., 1] = rs.uniform(3, 4, (n_steps, B))
    tot[..., 2] = 4.0
    tot[..., 3] = 9.0
    tot[..., 4] = 6.0 * np.asarray(p_target)[:, None]
    tot[..., 5] = rs.uniform(1, 2, (n_steps, B))
    w = rs.uniform(0.5, 1.5, (n_steps, B, S, 1))
    return tot[:, :, None, :] * (w / w.sum(axis=2, keepdims=True))


@pytest.mark.parametrize("p_target,diverged", [([0.99, 0.98, 0.97, 0.96], 4), ([0.90, 0.99, 0.99, 0.99], 0),
                                               ([0.99, 0.97, 0.94, 0.99], 2)])
@pytest.mark.parametrize("M,N", [(12, 16), (64, 64)])
def test_traj_metrics_from_hand_made_sums(be, p_target, diverged, M, N):
    B, n_steps = 3, 4
    _, S = _slices(be.lib, B, M, N, n_steps)
    sums = _hand_sums(p_target, B, S, np.random.RandomState(5)).astype(np.float32)
    m = _metrics(be, sums, B, M, N, n_steps)
    s = sums.astype(np.float64).sum(axis=2)
    step = (np.sqrt(s[..., 0]) / np.sqrt(s[..., 1])).mean(axis=1)
    corr = (s[..., 4] / (np.sqrt(s[..., 2]) * np.sqrt(s[..., 3]))).mean(axis=1)
    full = (np.sqrt(s[..., 5].sum(axis=0)) / np.sqrt(s[..., 3].sum(axis=0))).mean()
    assert m[2] == diverged                                                     # exact
    np.testing.assert_allclose(m[4:4 + n_steps], step, rtol=1e-6)
    np.testing.assert_allclose(m[4 + n_steps:], corr, atol=1e-6)
    np.testing.assert_allclose(m[4 + n_steps:], p_target, atol=1e-6)
    assert abs(m[0] - step.mean()) < 1e-6 * step.mean() and abs(m[1] - full) < 1e-6 * full and abs(m[3] - corr.mean()) < 1e-6


def test_traj_metrics_threshold_is_an_argument_and_nan_never_diverges(be):
    B, M, N, n_steps = 3, 12, 16, 4
    sums = _hand_sums([0.99, 0.97, 0.94, 0.99], B, 1, np.random.RandomState(6))
    assert _metrics(be, sums, B, M, N, n_steps, 0.98)[2] == 1
    assert _metrics(be, sums, B, M, N, n_steps, 0.5)[2] == 4
    sums[1, :, :, 2] = 0.0                                                      # p[1] = x / 0: not below any threshold (torch's `<`)
    sums[1, :, :, 4] = 0.0
    m = _metrics(be, sums, B, M, N, n_steps)
    assert np.isnan(m[4 + n_steps + 1]) and m[2] == 2


def test_step_then_metrics_end_to_end(be):
    """All n_steps launches, then the metrics, against the reference formulas in float64."""
    lib, p = be.lib, be.ptr
    B, M, N, T, n_steps = 3, 12, 16, 7, 4
    rs = np.random.RandomState(15)
    data = (rs.standard_normal((B, M, N, T)) + 0.3).astype(np.float32)
    outs = [(data[..., T - n_steps + t] + 0.1 * (t + 1) * rs.standard_normal((B, M, N))).astype(np.float32) for t in range(n_steps)]
    ws, S = _slices(lib, B, M, N, n_steps)
    d_im, d_preds, d_sums, d_data = be.empty((B, M, N)), be.empty((B, M, N, n_steps)), be.empty((ws,)), be.put(data)
    for t in range(n_steps):
        assert lib.ffno_markov_traj_step(p(be.put(outs[t])), None, None, p(d_data), p(d_im), p(d_preds), p(d_sums), B, M, N, T,
                                         n_steps, t, None) == 0
    d_m = be.empty((4 + 2 * n_steps,))
    assert lib.ffno_markov_traj_metrics(p(d_sums), p(d_m), B, M, N, n_steps, 0.95, None) == 0
    m = be.get(d_m).astype(np.float64)
    preds = np.stack(outs, axis=-1).astype(np.float64)
    assert np.array_equal(be.get(d_preds), np.stack(outs, axis=-1))
    yy = data[..., T - n_steps:].astype(np.float64)
    nrm = lambda a: np.sqrt((a ** 2).sum(axis=(1, 2)))       # noqa: E731   [B, n_steps]
    step = (nrm(preds - yy) / nrm(yy)).mean(axis=0)
    corr = ((preds * yy).sum(axis=(1, 2)) / (nrm(preds) * nrm(yy))).mean(axis=0)
    full = (np.sqrt(((preds - yy) ** 2).sum(axis=(1, 2, 3))) / np.sqrt((yy ** 2).sum(axis=(1, 2, 3)))).mean()
    np.testing.assert_allclose(m[4:4 + n_steps], step, rtol=5e-6)
    np.testing.assert_allclose(m[4 + n_steps:], corr, atol=5e-6)
    assert abs(m[0] - step.mean()) < 5e-6 * step.mean() and abs(m[1] - full) < 5e-6 * full
    below = np.nonzero(corr < 0.95)[0]
    assert np.abs(corr - 0.95).min() > 1e-3 and m[2] == (below[0] if len(below) else n_steps)
