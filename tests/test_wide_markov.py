"""Grid2DMarkovExperiment around a width-96 block: the routine's training step, validation, rollout() and simulate() on the
GEMM-composed wide engine (fourierflow_amd/engine_wide.py), and the shipped width-128 example config.  CPU wave emulator
(-m "not gpu") and MI355X (-m gpu)."""
import os

import numpy as np
import torch

import golden_util as gu
import oracle_util as ou
from backend_util import host_device, rel_l2  # noqa: F401
from oracle import ffno_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(modes=4, width=96, input_dim=3, n_layers=2, share_weight=True, factor=4, ff_weight_norm=True, gain=0.1)
SEED, B, G = 81, 2, 16


def routine(device):
    from fourierflow_amd.engine_wide import WideFFNO2DEngine
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    sd_np = gu.make_block_state_dict(KW, SEED)
    blk = FNOFactorized2DBlock(**KW)
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()})
    exp = Grid2DMarkovExperiment(blk.to(device), n_steps=3, max_accumulations=1, noise_std=0.01,
                                 scheduler=dict(num_warmup_steps=1, num_training_steps=10)).to(device)
    assert isinstance(exp.trainer().engine, WideFFNO2DEngine)
    return exp, sd_np


def batches(n):
    rs = np.random.RandomState(SEED)
    return [dict(x=(rs.standard_normal((B, G, G, 1)) * 3 + 1).astype(np.float32),
                 y=(rs.standard_normal((B, G, G, 1)) * 3 + 1).astype(np.float32),
                 noise=rs.standard_normal((B, G, G, 3)).astype(np.float32)) for _ in range(n)]


def test_wide_markov_training_step_is_the_oracle_composition(host_device):
    """Epoch 0 accumulates the statistics; the loss of one training step = orc.markov_features -> block -> inverse
    normalisation -> relative L2."""
    exp, sd_np = routine(host_device)
    dev = lambda a: torch.from_numpy(a).to(host_device)      # noqa: E731
    b0, b1 = batches(2)
    nz = orc.NormalizerState(3, max_accumulations=1)
    assert exp.training_step(dict(x=dev(b0["x"]), y=dev(b0["y"])), epoch=0, noise=dev(b0["noise"])) is None
    orc.markov_features(torch.tensor(b0["x"]), nz, torch.tensor(b0["noise"]), 0.01)
    loss = exp.training_step(dict(x=dev(b1["x"]), y=dev(b1["y"])), epoch=1, noise=dev(b1["noise"]))
    sd, _ = ou.torch_state_dict(sd_np, requires_grad=False)
    feats = orc.markov_features(torch.tensor(b1["x"]), nz, torch.tensor(b1["noise"]), 0.01)
    im = orc.ffno2d_block(sd, feats, modes=KW["modes"], n_layers=KW["n_layers"])["forecast"]
    ref = orc.lp_rel_loss(nz.inverse(im, 0), torch.tensor(b1["y"]))
    assert abs(loss.item() - ref.item()) < 1e-5
    assert exp.trainer().step_count == 1


def test_wide_markov_simulate_equals_explicit_steps_and_validation_runs(host_device):
    """simulate(x0, 3) (the engine + one fused advance launch per step) against rollout(x0, 3), which is three explicit
    feature / forward / inverse-normalisation steps; validation_step over a trajectory batch returns finite metrics."""
    exp, _ = routine(host_device)
    dev = lambda a: torch.from_numpy(a).to(host_device)      # noqa: E731
    b0, = batches(1)
    exp.training_step(dict(x=dev(b0["x"]), y=dev(b0["y"])), epoch=0, noise=dev(b0["noise"]))      # statistics
    x0 = dev(b0["x"][:1])
    want = exp.rollout(x0, 3)
    got = exp.simulate(x0, 3)
    assert tuple(got.shape) == (1, G, G, 3) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want) or rel_l2(got.cpu().numpy(), want.cpu().numpy()) < 1e-6
    rs = np.random.RandomState(SEED + 1)
    out = exp.validation_step({"data": dev(rs.standard_normal((1, G, G, 4)).astype(np.float32))})
    assert np.isfinite(float(out["valid_loss"])) and np.isfinite(float(out["valid_loss_avg"]))


def test_width128_example_config_builds_on_the_wide_engine():
    from fourierflow_amd.config import build_routine, load_config
    from fourierflow_amd.engine_wide import WideFFNO2DEngine
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    cfg = load_config(os.path.join(ROOT, "examples", "markov_width128.yaml"))
    exp = build_routine(cfg)
    assert isinstance(exp, Grid2DMarkovExperiment)
    assert (exp.conv.width, exp.conv.n_layers, exp.conv.modes, exp.conv.factor) == (128, 24, 16, 4)
    eng = exp.conv.engine()
    assert isinstance(eng, WideFFNO2DEngine) and (eng.C, eng.H, eng.L, eng.Ks) == (128, 512, 24, (16, 16))


def test_width128_example_trains_resumes_and_tests_through_the_cli(tmp_path, host_device):
    """`python -m fourierflow_amd train | test` on the example config (shrunk to two layers on an 8 x 8 grid): optimisation
    steps, the checkpoint with the wide engine's flat buffers, --resume and the test command."""
    import json
    import shutil

    from typer.testing import CliRunner

    from fourierflow_amd.cli import app
    cfg = tmp_path / "config.yaml"
    shutil.copy(os.path.join(ROOT, "examples", "markov_width128.yaml"), cfg)
    small = ["routine.conv.n_layers=2", "routine.conv.modes=4", "routine.conv.factor=2", "routine.n_steps=3", "builder.batch_size=1"]

    def run(*args):
        res = CliRunner().invoke(app, [*args, *small, "--grid", "8", "--device", host_device])
        assert res.exit_code == 0, (res.output, res.exception)
        return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]

    out = run("train", str(cfg), "--steps", "2", "--accumulation-batches", "1")
    assert [o["step"] for o in out[:-1]] == [0, 1] and all(np.isfinite(o["train_loss"]) for o in out[:-1])
    out = run("train", str(cfg), "--steps", "1", "--resume")
    assert out[0]["step"] == 2 and out[-1]["resumed_from_step"] == 2
    t = run("test", str(cfg), "--batches", "1")[-1]
    assert np.isfinite(t["test_loss"])
