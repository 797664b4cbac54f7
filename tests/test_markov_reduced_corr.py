"""Grid2DMarkovExperiment with ``downsample_corr=True``: the correlation on the grid of ``corr_data`` (reference
routines/grid_2d_markov.py:350-372 with utils/array.py:18-80) on the emulator and on the GPU, against tests/coarsen_oracle.py applied
in float64 to the routine's OWN predictions.  A 16 x 16 model, corr_data 8 x 8, three trajectories, four steps.

Tolerance on p_2.  The routine's coarse vorticity comes from the fp32 velocity launch (project bound 1e-5 relative L2,
tests/test_velocity.py) passed through the difference stencil, the oracle's from a float64 transform of the same prediction.
Measured max |p_2 - float64| over the two cases below (plain, use_velocity): emulator 1.20e-7 and 8.5e-8, MI355X 1.10e-7 and
3.5e-8 (profiles/kolmogorov_builder.md); p_2 is near 1 there, where one fp32 step is 6e-8.  TOL is 4 x the largest of the four,
for box-to-box and summation-order differences.
"""
import numpy as np
import pytest
import torch

import coarsen_oracle as co
from backend_util import host_device  # noqa: F401

B, G, M2, T, TC, N_STEPS, STEP = 3, 16, 8, 6, 5, 4, 0.5
LX, LY = 2 * np.pi, 2 * np.pi
TOL = 4 * 1.2e-7


def _routine(device, use_velocity, **kw):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    torch.manual_seed(5)
    blk = FNOFactorized2DBlock(modes=4, width=32, n_layers=1, input_dim=5 if use_velocity else 3, factor=2)
    exp = Grid2DMarkovExperiment(blk, n_steps=N_STEPS, step_size=STEP, grid_size=[G], use_velocity=use_velocity, noise_std=0.0,
                                 **kw).to(device)
    x = torch.from_numpy((np.random.RandomState(1).standard_normal((B, G, G, 1)) + 0.3).astype(np.float32)).to(device)
    exp.train()
    with torch.no_grad():
        exp._build_features({"x": x})      # the normaliser's statistics
    return exp.eval()


def _data(device):
    rs = np.random.RandomState(2)
    data = (rs.standard_normal((B, G, G, T)) + 0.3).astype(np.float32)
    times = np.tile(np.arange(T, dtype=np.float32) * STEP, (B, 1))
    return {"data": torch.from_numpy(data).to(device), "times": torch.from_numpy(times).to(device)}


def _own_preds(exp, batch):
    return exp._valid_step({k: v for k, v in batch.items() if k != "corr_data"})[2].cpu().numpy()


def _noisy_corr(wc, sigmas, seed):
    """corr_data [B, m, m, TC] whose last N_STEPS columns are wc[..., t] + sigma_t noise (in units of wc's spread)."""
    rs = np.random.RandomState(seed)
    corr = rs.standard_normal((B, M2, M2, TC))
    for t, s in enumerate(sigmas):
        corr[..., TC - N_STEPS + t] = wc[..., t] + s * wc[..., t].std() * rs.standard_normal((B, M2, M2))
    return corr.astype(np.float32)


@pytest.mark.parametrize("use_velocity", [False, True])
def test_reduced_metrics_match_the_oracle_on_the_routines_own_predictions(host_device, use_velocity):
    exp = _routine(host_device, use_velocity, downsample_corr=True)
    batch = _data(host_device)
    preds = _own_preds(exp, batch)
    wc = co.downsample_vorticity(preds, M2, LX, LY)
    corr = _noisy_corr(wc, (0.05, 0.2, 0.6, 2.0), 3)      # p_2 about 0.999, 0.98, 0.86, 0.45: diverged at step 2
    batch["corr_data"] = torch.from_numpy(corr).to(host_device)
    want, diverged = co.correlation(wc, corr, N_STEPS)
    assert diverged == 2 and np.abs(want - 0.95).min() > 1e-2
    loss_sum, step_losses, again, _ = exp._valid_step(batch)
    assert np.array_equal(again.cpu().numpy(), preds)      # the reduction leaves the rollout alone
    loss, loss_full, time_until, reduced, p, times = exp.compute_losses(batch, loss_sum, again)
    got = p.cpu().numpy().astype(np.float64)
    print(f"use_velocity={use_velocity}: max |p_2 - float64| {np.abs(got - want).max():.3e}")
    assert got.shape == (N_STEPS,) and np.abs(got - want).max() <= TOL
    assert reduced == diverged * STEP
    full_p, full_div = co.correlation(preds, batch["data"].cpu().numpy(), N_STEPS)      # the same formula on the model's grid
    assert time_until == full_div * STEP and np.abs(full_p - 0.95).min() > 1e-3      # time_until stays the full-resolution one
    assert np.array_equal(times.cpu().numpy(), np.arange(T - N_STEPS, T, dtype=np.float32) * STEP)
    v = exp.validation_step(batch)
    assert v["valid_reduced_time_until"] == diverged * STEP and v["valid_time_until"] == full_div * STEP
    assert abs(v["valid_corr"] - want.mean()) <= TOL
    t = exp.test_step(batch)
    assert np.array_equal(t["test_correlations"].cpu().numpy(), p.cpu().numpy()) and abs(t["test_corr"] - want.mean()) <= TOL
    assert t["test_reduced_time_until"] == diverged * STEP and t["test_time_until"] == full_div * STEP
    # foreign preds (not the cached tensor of the last _valid_step) take the same launches: the same bits
    loss_b, full_b, tu_b, red_b, p_b, _ = exp.compute_losses(batch, loss_sum, again.clone())
    assert np.array_equal(p_b.cpu().numpy(), p.cpu().numpy()) and (tu_b, red_b) == (time_until, reduced)
    assert float(full_b) == float(loss_full)


def test_reduced_correlation_diverges_while_the_full_one_never_does(host_device):
    """data holds the predictions themselves (full-resolution p = 1 at every step); corr_data is the oracle's reduction of the
    first prediction at step 0 and independent noise after."""
    exp = _routine(host_device, True, downsample_corr=True)
    batch = _data(host_device)
    preds = _own_preds(exp, batch)
    first = batch["data"].cpu().numpy()[..., T - N_STEPS - 1:T - N_STEPS]
    batch["data"] = torch.from_numpy(np.concatenate([first, preds], axis=-1)).to(host_device)
    batch["times"] = batch["times"][:, :N_STEPS + 1].contiguous()
    rs = np.random.RandomState(4)
    corr = rs.standard_normal((B, M2, M2, TC)).astype(np.float32)
    corr[..., TC - N_STEPS] = co.downsample_vorticity(preds[..., :1], M2, LX, LY)[..., 0]
    batch["corr_data"] = torch.from_numpy(corr).to(host_device)
    v = exp.validation_step(batch)
    assert v["valid_reduced_time_until"] == 1 * STEP and v["valid_time_until"] == N_STEPS * STEP
    p = exp.test_step(batch)["test_correlations"].cpu().numpy()
    assert abs(p[0] - 1.0) <= 1e-5 and np.abs(p[1:]).max() < 0.5


def test_switch_off_refuses_and_own_size_is_bit_equal_either_way(host_device):
    off, on = _routine(host_device, True), _routine(host_device, True, downsample_corr=True)
    batch = _data(host_device)
    small = dict(batch, corr_data=torch.zeros(B, M2, M2, TC, device=host_device))
    with pytest.raises(NotImplementedError, match="downsample_vorticity.*downsample_corr=True"):
        off.validation_step(small)
    same = dict(batch, corr_data=torch.from_numpy(np.random.RandomState(6).standard_normal((B, G, G, TC)).astype(np.float32))
                .to(host_device))
    a, b, c = off.test_step(same), on.test_step(same), off.test_step(batch)
    assert set(a) == set(b) == set(c)
    for k in a:
        for other in (b, c):      # corr_data at the model's own size changes nothing, with or without the switch
            if torch.is_tensor(a[k]):
                assert np.array_equal(a[k].cpu().numpy(), other[k].cpu().numpy()), k
            else:
                assert a[k] == other[k], k
    assert off.last_metrics.numel() == on.last_metrics.numel() == 4 + 2 * N_STEPS


@pytest.mark.parametrize("shape,words", [((B, M2, M2, N_STEPS - 1), ("3 steps", "compares 4")),
                                         ((B, 6, 6, TC), ("integer factor", "16 / 6")),
                                         ((B, M2, 4, TC), ("not square",))])
def test_corr_data_that_cannot_be_reduced_to_is_a_value_error(host_device, shape, words):
    exp = _routine(host_device, False, downsample_corr=True)
    batch = dict(_data(host_device), corr_data=torch.zeros(*shape, device=host_device))
    with pytest.raises(ValueError) as e:
        exp.validation_step(batch)
    for w in (*words, str(shape).replace(",)", ")")):
        assert w in str(e.value), (w, str(e.value))
