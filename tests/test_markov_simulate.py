"""Grid2DMarkovExperiment.simulate: the trained model as a simulator (the engine and one ffno_markov_advance launch per step)
against `_valid_step`, which runs the same forward engine on the same inputs and is itself pinned to the reference by
tests/test_markov_validation.py.  From the first input of a validation batch, with the batch's force maps and viscosities,
simulate returns `_valid_step`'s predictions BIT FOR BIT: the inverse affine is the same fused multiply-add, the features of the
next step come from the device code of ffno_markov_features (tests/test_kernels_markov_advance.py), and nothing else differs.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
from backend_util import host_device  # noqa: F401

B, G, T, N_STEPS = 3, 16, 7, 4
BLOCK = dict(modes=4, width=32, n_layers=2, share_weight=True, factor=4, ff_weight_norm=True, gain=0.1)
CASES = {
    "plain": dict(),
    "diff": dict(learn_difference=True),
    "force_mu": dict(append_force=True, append_mu=True),
    "force_mu_diff_raw": dict(append_force=True, append_mu=True, learn_difference=True, should_normalize=False, use_position=False),
    "velocity": dict(use_velocity=True),
    "shuffle": dict(shuffle_grid=True),
}


def _input_dim(flags):
    return (3 if flags.get("use_velocity") else 1) + (2 if flags.get("use_position", True) else 0) + \
        int(bool(flags.get("append_force"))) + int(bool(flags.get("append_mu")))


def _routine(tag, device):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    flags = CASES[tag]
    D = _input_dim(flags)
    kw = dict(BLOCK, input_dim=D)
    blk = FNOFactorized2DBlock(**kw)
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in gu.make_block_state_dict(kw, 70).items()})
    torch.manual_seed(5)      # the permutations of shuffle_grid
    exp = Grid2DMarkovExperiment(blk, n_steps=N_STEPS, step_size=0.5, grid_size=[G], **flags)
    if flags.get("should_normalize", True):      # statistics of a made-up accumulation: mean 0.2 c, variance (1 + 0.1 c)^2
        nz, c, count = exp.normalizer, torch.arange(D, dtype=torch.float32), 1000.0
        mean, std = 0.2 * c, 1.0 + 0.1 * c
        nz.sum.copy_((mean * count).reshape(nz.sum.shape))
        nz.sum_squared.copy_(((std ** 2 + mean ** 2) * count).reshape(nz.sum_squared.shape))
        nz.count.fill_(count)
        nz.n_accumulations.fill_(3.0)
        nz._n_acc_host = 3.0
    return exp.to(device)


def _batch(tag, device, t_force=T):
    rs = np.random.RandomState(71)
    b = {"data": rs.standard_normal((B, G, G, T)).astype(np.float32)}
    if CASES[tag].get("append_force"):
        b["f"] = rs.standard_normal((B, G, G, t_force)).astype(np.float32)      # one map per time: `_valid_step` takes the last n_steps
        b["mu"] = rs.uniform(0.1, 1.0, B).astype(np.float32)
    return {k: torch.from_numpy(v).to(device) for k, v in b.items()}


def _simulate_like_valid(exp, batch, n=N_STEPS, **kw):
    f = batch["f"][..., -n:] if "f" in batch else None      # a strided view of the stack: read in place
    return exp.simulate(batch["data"][..., T - n - 1:T - n], n, f, batch.get("mu"), **kw)


@pytest.mark.parametrize("tag", list(CASES))
def test_simulate_equals_the_validation_rollout_bit_for_bit(host_device, tag):
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    want = exp._valid_step(batch)[2]
    got = _simulate_like_valid(exp, batch)
    assert tuple(got.shape) == (B, G, G, N_STEPS) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want), float((got - want).abs().max())


def test_simulate_with_one_force_map_and_flat_x0(host_device):
    """f [B, M, N] stays fixed over the steps, as in rollout(); x0 may come without its channel axis."""
    exp = _routine("force_mu", host_device)
    batch = _batch("force_mu", host_device)
    f = batch["f"][..., 0].contiguous()
    want = exp._valid_step(dict(batch, f=f))[2]
    got = exp.simulate(batch["data"][..., T - N_STEPS - 1], N_STEPS, f, batch["mu"])
    assert torch.equal(got, want)


@pytest.mark.parametrize("tag", ["diff", "velocity"])
def test_every_keeps_every_second_state(host_device, tag):
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    full = _simulate_like_valid(exp, batch)
    half = _simulate_like_valid(exp, batch, every=2)
    assert tuple(half.shape) == (B, G, G, N_STEPS // 2)
    assert torch.equal(half, full[..., 1::2])
    assert torch.equal(_simulate_like_valid(exp, batch, every=N_STEPS)[..., 0], full[..., -1])


def test_simulate_leaves_the_normaliser_alone(host_device):
    exp = _routine("plain", host_device)
    batch = _batch("plain", host_device)
    for training in (True, False):
        exp.normalizer.train(training)
        state = {k: v.clone() for k, v in exp.normalizer.state_dict().items()}
        _simulate_like_valid(exp, batch)
        for k, v in exp.normalizer.state_dict().items():
            assert torch.equal(v, state[k]), k
        assert exp.normalizer.training is training
    exp.normalizer.train(True)

    def broken(*a, **k):
        raise RuntimeError("forward failed")

    exp.trainer().engine.forward = broken      # the flag comes back on an exception as well
    with pytest.raises(RuntimeError, match="forward failed"):
        _simulate_like_valid(exp, batch)
    assert exp.normalizer.training


@pytest.mark.parametrize("tag", ["plain", "force_mu"])
def test_simulate_refuses_wrong_shapes(host_device, tag):
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    x0 = batch["data"][..., 0]
    with pytest.raises(ValueError, match="x0"):
        exp.simulate(batch["data"][..., :2], N_STEPS, batch.get("f"), batch.get("mu"))
    for n, every in ((0, 1), (4, 0), (4, 3)):
        with pytest.raises(ValueError, match="every"):
            exp.simulate(x0, n, batch.get("f"), batch.get("mu"), every=every)
    if tag == "force_mu":
        f, mu = batch["f"], batch["mu"]
        for bad_f in (None, f[..., :N_STEPS - 1], f[:, :-1], f[:2, ..., 0], f[..., 0].reshape(B, G * G)):
            with pytest.raises(ValueError, match="f must be"):
                exp.simulate(x0, N_STEPS, bad_f, mu)
        for bad_mu in (None, mu[:2], mu.reshape(B, 1)):
            with pytest.raises(ValueError, match="mu must be"):
                exp.simulate(x0, N_STEPS, f, bad_mu)
        assert exp.normalizer.training
