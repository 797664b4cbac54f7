"""Trajectory validation of Grid2DMarkovExperiment (`_valid_step`, `compute_losses`, `validation_step`, `test_step`; reference
routines/grid_2d_markov.py:195-416) on the HIP path against a float64 restatement of the reference loop, for every case of
tests/golden/markov_valid.npz (tools/make_golden_markov_valid.py: a run of the reference's own method bodies over its real
FNOFactorized2DBlock, Normalizer and LpLoss).  The restatement is pinned to the reference by evaluating it in fp32 against the
fixture's outputs.

Bars: preds <= 1e-5 relative L2 (the project's forward bar); where the reference's own fp32 run sits further than 2.5e-6 from
the float64 restatement the bar is 4 x that distance (as oracle_util.check_grads_at_rounding_level does).  Losses 1e-5
relative, p 1e-5 absolute, time_until exact -- which needs every p[t] of the float64 restatement at least 1e-3 away from the
0.95 threshold, asserted before any kernel runs.
"""
import ast
import functools
import math

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle_util as ou
from backend_util import host_device, rel_l2  # noqa: F401
from oracle import ffno_oracle as orc

G = gu.load_golden("markov_valid")
B, M, N, T, N_STEPS = (int(v) for v in G["meta"])
BLOCK = ast.literal_eval(str(G["block"]))
DOMAIN = tuple(tuple(float(v) for v in d) for d in G["domain"])
CASES = [str(c) for c in G["cases"]]


def _flags(tag):
    return ast.literal_eval(str(G[f"{tag}.flags"]))


def _input_dim(flags):
    return (3 if flags.get("use_velocity") else 1) + 2 + int(bool(flags.get("append_force"))) + int(bool(flags.get("append_mu")))


def _batch_np(tag):
    b = {"data": G[f"{tag}.data"], "times": G[f"{tag}.times"]}
    for k in ("f", "mu"):
        if f"{tag}.{k}" in G.files:
            b[k] = G[f"{tag}.{k}"]
    return b


def restate_valid(sd_np, flags, batch, norm_state, step_size, dtype, n_steps=N_STEPS, perms=None):
    """The reference's `_valid_step` + `compute_losses` (:195-372) restated over the oracle's pieces, in `dtype`.
    norm_state = (sum, sum_squared, count) of the Normalizer or None; perms = (x_idx, y_idx) of shuffle_grid."""
    sd, _ = ou.torch_state_dict(sd_np, dtype=dtype, requires_grad=False)
    data = torch.tensor(batch["data"], dtype=dtype)
    Bn, _, _, Tn = data.shape
    D = _input_dim(flags)
    nz = None
    if flags.get("should_normalize", True):
        nz = orc.NormalizerState(D, dtype=dtype)
        nz.sum, nz.sum_squared, nz.count = (torch.tensor(np.asarray(v), dtype=dtype) for v in norm_state)
    force = torch.tensor(batch["f"], dtype=dtype) if flags.get("append_force") else None
    if force is not None and force.dim() == 4:
        force = force[..., -n_steps:]
    mu = torch.tensor(batch["mu"], dtype=dtype) if flags.get("append_mu") else None
    yy = data[..., -n_steps:]
    x = data[..., Tn - n_steps - 1].unsqueeze(-1)
    prev, preds, step_losses = x, [], []
    for t in range(n_steps):
        xin = orc.velocity_features(x, DOMAIN) if flags.get("use_velocity") else x
        f_t = None if force is None else (force if force.dim() == 3 else force[..., t])
        feats = orc.markov_features(xin, nz, None, 0.0, training=False, force=f_t, mu=mu)
        if perms is not None:
            feats = feats[:, perms[0]][:, :, perms[1]]
        im = orc.ffno2d_block(sd, feats, modes=BLOCK["modes"], n_layers=BLOCK["n_layers"])["forecast"]
        if perms is not None:
            im = im[:, :, torch.argsort(perms[1])][:, torch.argsort(perms[0])]
        if nz is not None:
            im = nz.inverse(im, 0)
        y = yy[..., t] - yy[..., t - 1] if flags.get("learn_difference") else yy[..., t]      # t = 0: index -1, as the reference
        step_losses.append(orc.lp_rel_loss(im.reshape(Bn, -1), y.reshape(Bn, -1)))
        if flags.get("learn_difference"):
            im = prev + im
            prev = im
        preds.append(im)
        x = im
    preds = torch.cat(preds, dim=-1)
    loss_full = orc.lp_rel_loss(preds.reshape(Bn, -1), yy.reshape(Bn, -1))
    p = ((preds / torch.norm(preds, dim=[1, 2], keepdim=True)) * (yy / torch.norm(yy, dim=[1, 2], keepdim=True)))
    p = p.sum(dim=[1, 2]).mean(dim=0)
    below = (p < 0.95).nonzero()
    diverged = int(below[0, 0]) if len(below) else n_steps
    return dict(preds=preds.numpy(), step_losses=np.array([float(l) for l in step_losses]),
                loss=float(sum(step_losses) / n_steps), loss_full=float(loss_full), p=p.numpy().astype(np.float64),
                time_until=diverged * step_size)


@functools.lru_cache(maxsize=None)
def _restated(tag, dtype):
    flags = _flags(tag)
    kw = dict(BLOCK, input_dim=_input_dim(flags))
    sd_np = gu.make_block_state_dict(kw, int(G[f"{tag}.seeds"][0]))
    norm = (G[f"{tag}.norm_sum"], G[f"{tag}.norm_sumsq"], G[f"{tag}.norm_count"])
    return restate_valid(sd_np, flags, _batch_np(tag), norm, float(G[f"{tag}.step_size"]), dtype)


def _routine(tag, device, **override):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    flags = dict(_flags(tag), **override)
    kw = dict(BLOCK, input_dim=_input_dim(flags))
    blk = FNOFactorized2DBlock(**kw)
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in gu.make_block_state_dict(kw, int(G[f"{tag}.seeds"][0])).items()})
    exp = Grid2DMarkovExperiment(blk, n_steps=N_STEPS, step_size=float(G[f"{tag}.step_size"]), grid_size=[M], domain=DOMAIN,
                                 n_test_steps_logged=2, heatmap_scale=3, pred_path=None, **flags)
    nz = exp.normalizer
    nz.sum.copy_(torch.from_numpy(G[f"{tag}.norm_sum"]))
    nz.sum_squared.copy_(torch.from_numpy(G[f"{tag}.norm_sumsq"]))
    nz.count.copy_(torch.from_numpy(G[f"{tag}.norm_count"]))
    nz.n_accumulations.copy_(torch.from_numpy(G[f"{tag}.norm_nacc"]))
    nz._n_acc_host = float(G[f"{tag}.norm_nacc"])
    return exp.to(device)


def _batch(tag, device):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in _batch_np(tag).items()}


# ---- the restatement is the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_restatement_in_fp32_reproduces_the_reference_run(tag):
    """Same op sequence, same precision: what is left is the order of fp32 operations inside the block (the oracle's einsum
    against the reference's) carried through four autoregressive steps."""
    r = _restated(tag, torch.float32)
    e = rel_l2(r["preds"], G[f"{tag}.preds"])
    print(f"{tag}: fp32 restatement vs reference run: preds {e:.2e}")
    assert e < 3e-6
    np.testing.assert_allclose(r["step_losses"], G[f"{tag}.step_losses"], rtol=3e-6)
    assert abs(r["loss"] - float(G[f"{tag}.loss"])) < 3e-6 * r["loss"]
    assert abs(r["loss_full"] - float(G[f"{tag}.loss_full"])) < 3e-6 * r["loss_full"]
    np.testing.assert_allclose(r["p"], G[f"{tag}.p"], atol=2e-6)
    assert r["time_until"] == float(G[f"{tag}.time_until"])


def test_fixture_covers_the_three_divergence_cases():
    step = {tag: float(G[f"{tag}.time_until"]) / float(G[f"{tag}.step_size"]) for tag in CASES}
    assert step["interior"] == 2 and step["never"] == N_STEPS and step["at_zero"] == 0
    assert float(G["interior.step_size"]) != 1.0 and float(G["never.time_until"]) == N_STEPS * float(G["never.step_size"])
    assert G["force_mu.f"].ndim == 4 and G["force_mu.f"].shape[-1] > N_STEPS and T - N_STEPS - 1 > 0


# ---- the HIP routine -------------------------------------------------------------------------------------------------------------
def _check_against_restatement(tag, loss, loss_full, time_until, reduced, p, preds):
    r64 = _restated(tag, torch.float64)
    assert np.abs(r64["p"] - 0.95).min() >= 1e-3            # precondition on the oracle alone
    noise = rel_l2(G[f"{tag}.preds"], r64["preds"])         # the reference's own fp32 run against float64
    bar = 1e-5 if noise <= 2.5e-6 else 4 * noise
    e = rel_l2(preds, r64["preds"])
    print(f"{tag}: preds vs float64 {e:.2e} (reference fp32 run: {noise:.2e}, bar {bar:.2e}); loss {abs(loss - r64['loss']) / r64['loss']:.2e} "
          f"loss_full {abs(loss_full - r64['loss_full']) / r64['loss_full']:.2e} p {np.abs(p - r64['p']).max():.2e}")
    assert e <= bar
    assert abs(loss - r64["loss"]) <= 1e-5 * r64["loss"] and abs(loss_full - r64["loss_full"]) <= 1e-5 * r64["loss_full"]
    assert np.abs(p - r64["p"]).max() <= 1e-5
    assert time_until == r64["time_until"] == float(G[f"{tag}.time_until"]) and reduced == time_until
    return r64


@pytest.mark.parametrize("tag", CASES)
def test_valid_step_and_compute_losses_match_float64(host_device, tag):
    exp = _routine(tag, host_device)
    r64 = _restated(tag, torch.float64)
    assert np.abs(r64["p"] - 0.95).min() >= 1e-3
    batch = _batch(tag, host_device)
    batch["corr_data"] = batch["data"]                      # the grid's own size: reduced metrics = the full ones
    state = {k: v.clone() for k, v in exp.normalizer.state_dict().items()}
    loss_sum, step_losses, preds, layers = exp._valid_step(batch)
    assert tuple(preds.shape) == (B, M, N, N_STEPS) and layers == [] and len(step_losses) == N_STEPS
    np.testing.assert_allclose(step_losses.cpu().numpy(), r64["step_losses"], rtol=1e-5)
    assert abs(float(loss_sum) - r64["step_losses"].sum()) <= 1e-5 * r64["step_losses"].sum()
    loss, loss_full, time_until, reduced, p, times = exp.compute_losses(batch, loss_sum, preds)
    _check_against_restatement(tag, float(loss), float(loss_full), time_until, reduced, p.cpu().numpy().astype(np.float64),
                               preds.cpu().numpy())
    assert np.array_equal(times.cpu().numpy(), G[f"{tag}.ref_times"])
    for k, v in exp.normalizer.state_dict().items():        # validation never accumulates: bit-identical statistics
        assert torch.equal(v, state[k]), k
    assert exp.normalizer.training                           # and the mode it was called in is restored


@pytest.mark.parametrize("tag", CASES)
def test_validation_and_test_step_keys_and_values(host_device, tag):
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    v = exp.validation_step(batch, 0)
    assert set(v) == {"valid_loss_avg", "valid_loss", "valid_time_until", "valid_reduced_time_until", "valid_corr"}
    r64 = _check_against_restatement(tag, float(v["valid_loss_avg"]), float(v["valid_loss"]), v["valid_time_until"],
                                     v["valid_reduced_time_until"], exp._traj[1][4 + N_STEPS:].cpu().numpy().astype(np.float64),
                                     exp._traj[0].cpu().numpy())
    assert abs(v["valid_corr"] - r64["p"].mean()) <= 1e-5
    t = exp.test_step(batch, 0)
    assert {"test_loss_avg", "test_loss", "test_time_until", "test_reduced_time_until", "test_corr", "test_correlations",
            "test_losses"} <= set(t)
    assert float(t["test_loss"]) == float(v["valid_loss"]) and float(t["test_loss_avg"]) == float(v["valid_loss_avg"])   # deterministic
    assert t["test_time_until"] == v["valid_time_until"]
    np.testing.assert_allclose(t["test_correlations"].cpu().numpy(), r64["p"], atol=1e-5)
    np.testing.assert_allclose(t["test_losses"].cpu().numpy(), r64["step_losses"], rtol=1e-5)


def test_compute_losses_on_foreign_preds_runs_the_same_kernels(host_device):
    """`preds` that did not come from the last `_valid_step` (here: the reference's own) are reduced by the same two kernels."""
    tag = "interior"
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    preds = torch.from_numpy(G[f"{tag}.preds"].copy()).to(host_device)
    loss_sum = torch.tensor(float(G[f"{tag}.loss_sum"]), device=host_device)
    loss, loss_full, time_until, reduced, p, _ = exp.compute_losses(batch, loss_sum, preds)
    assert abs(float(loss) - float(G[f"{tag}.loss"])) <= 1e-5 * float(G[f"{tag}.loss"])
    assert abs(float(loss_full) - float(G[f"{tag}.loss_full"])) <= 1e-5 * float(G[f"{tag}.loss_full"])
    np.testing.assert_allclose(p.cpu().numpy(), G[f"{tag}.p"], atol=1e-5)
    assert time_until == reduced == float(G[f"{tag}.time_until"]) == 2 * 0.25


def test_step_size_is_stored_and_scales_time_until(host_device):
    a, b = _routine("interior", host_device), _routine("never", host_device)
    assert a.step_size == 0.25 and b.step_size == 0.5
    assert a.validation_step(_batch("interior", host_device))["valid_time_until"] == 2 * 0.25
    assert b.validation_step(_batch("never", host_device))["valid_time_until"] == N_STEPS * 0.5
    a.step_size = 3.0
    assert a.test_step(_batch("interior", host_device))["test_time_until"] == 6.0


def test_n_steps_defaults_to_the_whole_trajectory(host_device):
    exp = _routine("plain", host_device)
    exp.n_steps = None
    batch = _batch("plain", host_device)
    _, step_losses, preds, _ = exp._valid_step(batch)
    assert tuple(preds.shape) == (B, M, N, T - 1) and len(step_losses) == T - 1
    flags = _flags("plain")
    kw = dict(BLOCK, input_dim=_input_dim(flags))
    r = restate_valid(gu.make_block_state_dict(kw, int(G["plain.seeds"][0])), flags, _batch_np("plain"),
                      (G["plain.norm_sum"], G["plain.norm_sumsq"], G["plain.norm_count"]), 1.0, torch.float64, n_steps=T - 1)
    assert rel_l2(preds.cpu().numpy(), r["preds"]) <= 1e-5


def test_nan_rule_holds_for_validation_only(host_device):
    """:397-400: validation_step reports 9999.9 for a NaN loss (checkpoint selection); test_step reports the NaN."""
    exp = _routine("plain", host_device)
    batch = _batch("plain", host_device)
    batch["data"] = batch["data"].clone()
    batch["data"][1, 3, 5, T - 1] = float("nan")          # in the last target only: the rollout itself stays finite
    v = exp.validation_step(batch)
    assert v["valid_loss_avg"] == 9999.9 and v["valid_loss"] == 9999.9
    t = exp.test_step(batch)
    assert math.isnan(float(t["test_loss_avg"])) and math.isnan(float(t["test_loss"]))
    assert bool(torch.isfinite(exp._traj[0]).all())


def test_corr_data_of_another_size_raises(host_device):
    exp = _routine("plain", host_device)
    batch = _batch("plain", host_device)
    batch["corr_data"] = torch.zeros(B, M // 2, N // 2, T, device=host_device)
    loss_sum, _, preds, _ = exp._valid_step(batch)
    with pytest.raises(NotImplementedError, match="downsample_vorticity"):
        exp.compute_losses(batch, loss_sum, preds)
    with pytest.raises(NotImplementedError, match="downsample_vorticity"):
        exp.validation_step(batch)


@pytest.mark.parametrize("tag", ["plain", "diff", "force_mu"])
def test_rollout_agrees_with_the_validation_predictions(host_device, tag):
    """`rollout()` keeps its signature and results: from the same first input it returns the `preds` of `_valid_step` (its
    inverse normalisation is the unfused `im * std + mean`: one rounding of the product apart)."""
    exp = _routine(tag, host_device)
    batch = _batch(tag, host_device)
    x0 = batch["data"][..., T - N_STEPS - 1].unsqueeze(-1).contiguous()
    f = batch["f"][..., -1].contiguous() if "f" in batch else None          # rollout keeps one force map: compare step 0 only
    roll = exp.rollout(x0, N_STEPS, f, batch.get("mu"))
    preds = exp._valid_step(batch)[2]
    assert tuple(roll.shape) == tuple(preds.shape)
    if f is None:
        assert rel_l2(roll.cpu().numpy(), preds.cpu().numpy()) < 1e-6
    else:
        f0 = batch["f"][..., -N_STEPS].contiguous()
        roll = exp.rollout(x0, 1, f0, batch.get("mu"))
        assert rel_l2(roll.cpu().numpy(), preds[..., :1].cpu().numpy()) < 1e-6


def test_shuffled_grid_goes_through_the_permutations(host_device):
    """shuffle_grid (:297-304) on a square grid, against the restatement with the routine's own permutations."""
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    Gs, Ts = 12, 5
    kw = dict(BLOCK, input_dim=3)
    sd_np = gu.make_block_state_dict(kw, 91)
    blk = FNOFactorized2DBlock(**kw)
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
    torch.manual_seed(4)
    exp = Grid2DMarkovExperiment(blk, should_normalize=False, shuffle_grid=True, grid_size=[Gs]).to(host_device)
    rs = np.random.RandomState(92)
    data = rs.standard_normal((B, Gs, Gs, Ts)).astype(np.float32)
    r = restate_valid(sd_np, dict(should_normalize=False), {"data": data}, None, 1.0, torch.float64, n_steps=Ts - 1,
                      perms=(exp._x_idx.cpu(), exp._y_idx.cpu()))
    _, step_losses, preds, _ = exp._valid_step({"data": torch.from_numpy(data).to(host_device)})
    assert rel_l2(preds.cpu().numpy(), r["preds"]) <= 1e-5
    np.testing.assert_allclose(step_losses.cpu().numpy(), r["step_losses"], rtol=1e-5)
