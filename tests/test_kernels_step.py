"""The kernels that turn a gradient into a parameter change (pointwise.hip: ffno_adamw_flat, ffno_adam_flat, ffno_lploss_fwd_bwd,
ffno_axpy; glin.hip: the dropout keep set) through the C ABI against plain fp64 models -- on the CPU wave emulator (-m "not gpu")
and on the MI355X (-m gpu).

The optimiser is compared on the UPDATE p_new - p_old and on m and v after every step, not on the parameters: a decay of
lr wd = 1e-3 per step is 1e-3 of a parameter but 1e-1 of an update.  Reference: tests/step_models.adam_model in fp64 on a
trajectory of its own (same start, same gradients); floor: the same transcription in fp32 against it.

Worst measured rel-L2 against the fp64 model over the steps and both decay kinds (update / m / v); ADAM_BOUND is four times
the larger of the two backends, the factor covering fused multiply-add contraction and operation order:
    case    fp32 numpy floor                 emulator                         MI355X
    first   7.87e-06 / 5.90e-08 / 6.34e-08   7.32e-06 / 5.74e-08 / 6.35e-08   7.31e-06 / 5.75e-08 / 6.35e-08
    late    1.76e-05 / 6.98e-08 / 6.52e-08   1.77e-05 / 6.98e-08 / 6.52e-08   1.77e-05 / 6.98e-08 / 6.52e-08
    eps     2.04e-05 / 5.53e-08 / 7.92e-08   2.03e-05 / 5.53e-08 / 6.70e-08   2.03e-05 / 5.53e-08 / 6.69e-08
    wrap    1.75e-05 / 7.04e-08 / 6.37e-08   1.75e-05 / 7.04e-08 / 6.37e-08   1.75e-05 / 7.04e-08 / 6.37e-08
(wrap = the late inputs at n = 2048 * 256 + 4099: the grid of 2048 workgroups makes a second, ragged pass.)

ffno_lploss_fwd_bwd at gscale 20, affine (1.7, -0.4), B = 3, worst over the four sizes (bounds 1e-6 absolute / 1e-5 rel-L2):
    loss      emulator 5.2e-8   MI355X 5.2e-8
    gradient  emulator 1.1e-7   MI355X 1.1e-7
"""
import functools

import numpy as np
import pytest

from backend_util import be, rel_l2  # noqa: F401
from step_models import TERMS, adam_model, f32, keep_model, keep_threshold

N_RAGGED = 4099                     # 17 workgroups of 256, the last one holds 3 elements
N_WRAP = 2048 * 256 + 4099          # the grid is capped at 2048 workgroups: one full pass and a ragged second one
BETA1, BETA2 = 0.9, 0.999

#        lr    wd   grad_scale eps   gradient size  first step  given state
CASES = {
    "first": (1e-2, 0.1, 0.5, 1e-8, 1.0, 1, False),
    "late": (1e-2, 0.1, 0.5, 1e-8, 1.0, 997, True),
    "eps": (1e-2, 0.1, 0.5, 1e-3, 1e-3, 1, False),
}
N_STEPS = 4

# worst measured rel-L2 (update, m, v) per backend, to three digits (module docstring) ...
ADAM_MEASURED = {
    "first": {"emu": (7.32e-06, 5.74e-08, 6.35e-08), "gpu": (7.31e-06, 5.75e-08, 6.35e-08)},
    "late": {"emu": (1.77e-05, 6.98e-08, 6.52e-08), "gpu": (1.77e-05, 6.98e-08, 6.52e-08)},
    "eps": {"emu": (2.03e-05, 5.53e-08, 6.70e-08), "gpu": (2.03e-05, 5.53e-08, 6.69e-08)},
    "wrap": {"emu": (1.75e-05, 7.04e-08, 6.37e-08), "gpu": (1.75e-05, 7.04e-08, 6.37e-08)},
}
# ... and the bounds: four times the larger of the two
ADAM_BOUND = {k: tuple(4 * max(e, g) for e, g in zip(v["emu"], v["gpu"])) for k, v in ADAM_MEASURED.items()}


@functools.lru_cache(maxsize=None)
def adam_inputs(case, n):
    """-> p0, m0, v0, [g of each step] in fp32; read-only, shared by every test of the case."""
    _, _, _, _, gsize, _, given = CASES[case]
    rs = np.random.RandomState(sorted(CASES).index(case) * 7919 + n % 1000)
    p0 = rs.standard_normal(n).astype(np.float32)
    m0 = (0.3 * rs.standard_normal(n)).astype(np.float32) if given else np.zeros(n, np.float32)
    v0 = rs.uniform(0.2, 2.0, n).astype(np.float32) if given else np.zeros(n, np.float32)
    gs = [(gsize * rs.standard_normal(n)).astype(np.float32) for _ in range(N_STEPS)]
    for a in [p0, m0, v0] + gs:
        a.setflags(write=False)
    return p0, m0, v0, gs


@functools.lru_cache(maxsize=None)
def adam_trajectory(case, n, decoupled, dtype=np.float64, without=None):
    """-> [(update, m, v) after each step] of the model on its own trajectory."""
    lr, wd, gscale, eps, _, first, _ = CASES[case]
    p, m, v, gs = adam_inputs(case, n)
    p, m, v = (np.asarray(a, dtype) for a in (p, m, v))
    out = []
    for k, g in enumerate(gs):
        pn, m, v = adam_model(p, g, m, v, first + k, lr, BETA1, BETA2, eps, wd, gscale, decoupled, dtype, without)
        out.append((pn.astype(np.float64) - p.astype(np.float64), m, v))
        p = pn
    return out


def worst_errors(traj, ref):
    return tuple(max(rel_l2(t[q], r[q]) for t, r in zip(traj, ref)) for q in range(3))


def check_inputs_separate_every_term():
    """The condition on the inputs, in numpy only: leaving any one term out of the fp64 model moves the update or m by at least
    100 bounds in at least one of the three cases, for either decay kind.  (grad_scale shows only in m for first / decoupled:
    Adam's update is invariant under a scale of the gradient except through eps.)"""
    for decoupled in (1, 0):
        for term in TERMS:
            margin = 0.0
            for case in CASES:
                full = adam_trajectory(case, N_RAGGED, decoupled)
                dist = worst_errors(adam_trajectory(case, N_RAGGED, decoupled, np.float64, term), full)
                bound = ADAM_BOUND[case]
                margin = max(margin, dist[0] / bound[0], dist[1] / bound[1])
            assert margin >= 100, (decoupled, term, margin)


def test_adam_inputs_separate_every_term():
    check_inputs_separate_every_term()


def run_adam(be, case, n, decoupled):
    """The kernel on the case's inputs -> [(update, m, v) after each step]."""
    lib, p = be.lib, be.ptr
    lr, wd, gscale, eps, _, first, _ = CASES[case]
    p0, m0, v0, gs = adam_inputs(case, n)
    dp, dm, dv = be.put(p0), be.put(m0), be.put(v0)
    fn = lib.ffno_adamw_flat if decoupled else lib.ffno_adam_flat
    out, prev = [], p0.astype(np.float64)
    for k, g in enumerate(gs):
        assert fn(p(dp), p(be.put(g)), p(dm), p(dv), n, lr, BETA1, BETA2, eps, wd, first + k, gscale, None) == 0
        now = np.array(be.get(dp), np.float64)
        out.append((now - prev, np.array(be.get(dm)), np.array(be.get(dv))))
        prev = now
    return out


def assert_adam(be, case, n, decoupled, bound_key):
    ref = adam_trajectory(case, n, decoupled)
    floor = worst_errors(adam_trajectory(case, n, decoupled, np.float32), ref)
    got = worst_errors(run_adam(be, case, n, decoupled), ref)
    print(f"\nadam {bound_key} decoupled={decoupled} {be.kind}: update/m/v " + " / ".join(f"{e:.2e}" for e in got)
          + "   fp32 floor " + " / ".join(f"{e:.2e}" for e in floor))
    for name, e, b in zip(("update", "m", "v"), got, ADAM_BOUND[bound_key]):
        assert e < b, (name, e, b)


@pytest.mark.parametrize("decoupled", [1, 0])
@pytest.mark.parametrize("case", list(CASES))
def test_adam_step_against_fp64_model(be, case, decoupled):
    check_inputs_separate_every_term()
    assert_adam(be, case, N_RAGGED, decoupled, case)


@pytest.mark.parametrize("decoupled", [1, 0])
def test_adam_step_where_the_grid_stride_wraps(be, decoupled):
    assert (N_WRAP + 255) // 256 > 2048 and N_WRAP % 256 != 0
    assert_adam(be, "late", N_WRAP, decoupled, "wrap")


def test_adam_argument_checks(be):
    lib, p = be.lib, be.ptr
    a = be.zeros(8)
    for fn in (lib.ffno_adamw_flat, lib.ffno_adam_flat):
        assert fn(p(a), p(a), p(a), p(a), 8, 1e-2, BETA1, BETA2, 1e-8, 0.1, 0, 1.0, None) == -1       # step counts from 1
        assert fn(p(a), p(a), p(a), p(a), 0, 1e-2, BETA1, BETA2, 1e-8, 0.1, 1, 1.0, None) == -1
        assert fn(p(a), None, p(a), p(a), 8, 1e-2, BETA1, BETA2, 1e-8, 0.1, 1, 1.0, None) == -1


# ---- relative L2 loss ------------------------------------------------------------------------------------------------------------
LOSS_B, LOSS_GSCALE, LOSS_AFFINE = 3, 20.0, (1.7, -0.4)
LOSS_EXACT = 1                      # the sample whose prediction equals its target


def slices(n):
    return max(1, min(64, (n + 1023) // 1024))


@functools.lru_cache(maxsize=None)
def loss_case(n):
    """-> pred, target (fp32) and the fp64 torch reference (loss, gradient of gscale * loss) of LpLoss.rel on sc * pred + sh."""
    import torch
    B = LOSS_B
    sc, sh = (f32(a) for a in LOSS_AFFINE)
    rs = np.random.RandomState(n % 9973)
    pred = rs.standard_normal((B, n)).astype(np.float32)
    tgt = rs.standard_normal((B, n)).astype(np.float32)
    # the exact sample: predictions on a grid of 1/64 make sc * pred + sh exact in fp64 (33 significant bits at most), so its
    # rounding to fp32 is the kernel's single-rounding fused multiply-add and the difference is exactly zero there
    pred[LOSS_EXACT] = np.round(pred[LOSS_EXACT] * 64) / 64
    tgt[LOSS_EXACT] = (pred[LOSS_EXACT].astype(np.float64) * sc + sh).astype(np.float32)
    assert np.all(tgt[LOSS_EXACT] != 0)
    pt = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(tgt, dtype=torch.float64)
    l = ((pt * sc + sh - tt).norm(dim=1) / tt.norm(dim=1)).mean()       # LpLoss.rel
    (LOSS_GSCALE * l).backward()
    grad = pt.grad.numpy().copy()
    for a in (pred, tgt, grad):
        a.setflags(write=False)
    return pred, tgt, l.item(), grad


@pytest.mark.parametrize("n", [1, 1025, 20000, 70001])      # one slice / 513 + 512 / 20 slices / 64 slices of 1094 (the cap)
def test_lploss_scaled_and_shifted(be, n):
    lib, p = be.lib, be.ptr
    B = LOSS_B
    pred, tgt, ref_loss, ref_grad = loss_case(n)
    ntmp = lib.ffno_lploss_tmp_floats(B, n)
    assert ntmp == 2 * B * slices(n)
    assert {1: 1, 1025: 2, 20000: 20, 70001: 64}[n] == slices(n) and (n != 70001 or -(-n // 64) > 1024)
    dpred, dtgt, aff = be.put(pred), be.put(tgt), be.put(np.array(LOSS_AFFINE, np.float32))
    nan = lambda a: np.isnan(np.asarray(be.get(a))).all()      # noqa: E731
    other = np.arange(B) != LOSS_EXACT

    def check_loss(loss):
        got = float(be.get(loss)[0])
        print(f"\nlploss n={n} {be.kind}: loss error {abs(got - ref_loss):.2e}")
        assert np.isfinite(got) and abs(got - ref_loss) < 1e-6

    def check_grad(gp):
        got = np.asarray(be.get(gp))
        # the exact sample is left out of the comparison: in fp64 its difference is the fp32 rounding of the target (a unit
        # vector after normalisation), in the kernel's arithmetic it is zero
        print(f"\nlploss n={n} {be.kind}: gradient rel-L2 {rel_l2(got[other], ref_grad[other]):.2e}")
        assert rel_l2(got[other], ref_grad[other]) < 1e-5
        assert np.array_equal(got[LOSS_EXACT], np.zeros(n, np.float32))

    # both outputs (the work buffer arrives NaN-filled: every word that is read has been written by the first stage)
    loss, gp, tmp = be.empty(1), be.empty((B, n)), be.empty(ntmp)
    assert lib.ffno_lploss_fwd_bwd(p(dpred), p(dtgt), p(loss), p(gp), p(tmp), B, n, LOSS_GSCALE, p(aff), None) == 0
    check_loss(loss)
    check_grad(gp)
    # loss only: the gradient buffer stays as it was
    loss, gp, tmp = be.empty(1), be.empty((B, n)), be.empty(ntmp)
    assert lib.ffno_lploss_fwd_bwd(p(dpred), p(dtgt), p(loss), None, p(tmp), B, n, LOSS_GSCALE, p(aff), None) == 0
    check_loss(loss)
    assert nan(gp)
    # gradient only: the loss stays as it was
    loss2 = be.empty(1)
    assert lib.ffno_lploss_fwd_bwd(p(dpred), p(dtgt), None, p(gp), p(tmp), B, n, LOSS_GSCALE, p(aff), None) == 0
    check_grad(gp)
    assert nan(loss2) and not nan(loss)


# ---- sums ------------------------------------------------------------------------------------------------------------------------
def test_axpy_where_the_grid_stride_wraps(be):
    lib, p = be.lib, be.ptr
    n, alpha = N_WRAP, f32(-0.37)
    rs = np.random.RandomState(3)
    y = rs.standard_normal(n).astype(np.float32)
    x = rs.standard_normal(n).astype(np.float32)
    dy, dx = be.put(y), be.put(x)
    assert lib.ffno_axpy(p(dy), p(dx), alpha, n, None) == 0
    ref = y.astype(np.float64) + alpha * x.astype(np.float64)
    # one fused multiply-add = one rounding: half an ulp of the result, and |result| <= |y| + |alpha x|
    err = np.abs(np.asarray(be.get(dy), np.float64) - ref)
    assert np.all(err <= 2.0 ** -23 * (np.abs(y).astype(np.float64) + np.abs(alpha * x.astype(np.float64))))
    np.testing.assert_array_equal(be.get(dx), x)


# ---- dropout keep set ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_drop,seed", [(0.3, 1234), (0.25, 77), (0.999, 0), (1e-3, 0xFFFFFFFF)])
def test_dropout_mask_is_the_two_round_hash(be, p_drop, seed):
    n = 70001
    assert keep_threshold(p_drop) == min(2 ** 32 - 1, int(np.float64(np.float32(p_drop)) * 2.0 ** 32))
    m = be.zeros(n, np.uint8)
    assert be.lib.ffno_dropout_mask(be.ptr(m), n, p_drop, seed, None) == 0
    want = keep_model(n, p_drop, seed)
    np.testing.assert_array_equal(np.asarray(be.get(m)), want.astype(np.uint8))
    kept = want.mean()
    assert abs(kept - (1 - p_drop)) < 5 * np.sqrt(p_drop * (1 - p_drop) / n)         # (the model itself is a coin of bias p)
