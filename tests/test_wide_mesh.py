"""FNOFactorizedMesh2D / FNOFactorizedMesh3D at widths 96 / 128: the GEMM-composed wide mesh engine
(fourierflow_amd/engine_wide.py: WideFFNOMeshEngine over csrc/bgemm.hip and the pad / crop kernels of csrc/meshpad.hip) against
the oracle, the reference's state-dict layout, an AdamW run and the shipped width-128 example config -- on the CPU wave emulator
(-m "not gpu") and on the MI355X (-m gpu).  The method and the bars are those of test_wide_block.py."""
import io
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle_util as ou
from backend_util import host_device, rel_l2  # noqa: F401
from oracle import ffno_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_COMMON = dict(n_layers=2, n_ff_layers=2, layer_norm=False)
# 2-D: grid 5 x 4 padded by the module's 8 to 13 x 12 (13 is prime)
M2_W96 = dict(modes_x=3, modes_y=2, width=96, input_dim=4, share_weight=False, factor=4, ff_weight_norm=True, **_COMMON)
M2_W128 = dict(modes_x=3, modes_y=2, width=128, input_dim=4, share_weight=True, factor=2, ff_weight_norm=False, **_COMMON)
# 3-D: grid 3 x 4 x 2 padded by 2 to 5 x 6 x 4: K = S // 2 on every axis (the mode bound itself), first and last axes differ
M3_W96 = dict(modes_x=2, modes_y=3, modes_z=2, width=96, input_dim=5, output_dim=4, share_weight=False, factor=4,
              ff_weight_norm=True, **_COMMON)
# 3-D, the real padding: grid 5 x 3 x 4 padded by 8 to 13 x 11 x 12
M3_W128 = dict(modes_x=4, modes_y=3, modes_z=2, width=128, input_dim=5, output_dim=4, share_weight=True, factor=2,
               ff_weight_norm=True, **_COMMON)

CASES = {"2d_w96_unshared_f4": (M2_W96, 41, 2, (5, 4), 8), "2d_w128_shared_f2": (M2_W128, 42, 2, (5, 4), 8),
         "3d_w96_unshared_pad2": (M3_W96, 43, 2, (3, 4, 2), 2), "3d_w128_shared_pad8": (M3_W128, 44, 2, (5, 3, 4), 8)}


def _kind(kw):
    return 3 if "modes_z" in kw else 2


def modes_of(kw):
    return tuple(kw[k] for k in ("modes_x", "modes_y", "modes_z")[:_kind(kw)])


def state_dict_np(kw, seed):
    return (gu.make_mesh3d_state_dict if _kind(kw) == 3 else gu.make_mesh2d_state_dict)(kw, seed)


def make_io(kw, seed, B, S):
    return (gu.make_mesh3d_io if _kind(kw) == 3 else gu.make_mesh2d_io)(kw, seed, B, S)


def build_model(kw, seed, device, padding=8):
    from fourierflow_amd.modules import FNOFactorizedMesh2D, FNOFactorizedMesh3D
    blk = (FNOFactorizedMesh3D if _kind(kw) == 3 else FNOFactorizedMesh2D)(**kw)
    blk.padding = padding      # (read at the first engine() call)
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state_dict_np(kw, seed).items()}, strict=True)
    return blk.to(device)


def oracle_forward(kw, sd, x, padding, relu_masks=None):
    fn = orc.ffno_mesh3d if _kind(kw) == 3 else orc.ffno_mesh2d
    return fn(sd, x, modes=modes_of(kw), n_layers=kw["n_layers"], padding=padding, relu_masks=relu_masks)


def oracle_run(kw, seed, B, S, padding, dtype=torch.float32, relu_masks=None):
    """-> (output, loss, {parameter: gradient}, input gradient) of the oracle under the relative-L2 loss."""
    sd, uniq = ou.torch_state_dict(state_dict_np(kw, seed), dtype)
    x_np, t_np = make_io(kw, seed, B, S)
    x = torch.tensor(x_np, dtype=dtype, requires_grad=True)
    out = oracle_forward(kw, sd, x, padding, relu_masks)
    loss = orc.lp_rel_loss(out, torch.tensor(t_np, dtype=dtype))
    loss.backward()
    return out.detach(), loss.detach(), {k: p.grad.numpy() for k, p in uniq.items()}, x.grad.numpy()


def check_forward_and_every_gradient(tag, device):
    from fourierflow_amd.engine_wide import WideFFNOMeshEngine
    kw, seed, B, S, padding = CASES[tag]
    blk = build_model(kw, seed, device, padding)
    eng = blk.engine()
    assert isinstance(eng, WideFFNOMeshEngine) and eng.pad == padding
    x_np, t_np = make_io(kw, seed, B, S)
    x = torch.from_numpy(x_np).to(device).requires_grad_(True)
    pred = blk(x)
    assert tuple(pred.shape) == (B, *S, kw.get("output_dim", 1))
    loss = orc.lp_rel_loss(pred, torch.from_numpy(t_np).to(device))
    loss.backward()
    ref_out, ref_loss, _, _ = oracle_run(kw, seed, B, S, padding)
    e = rel_l2(pred.detach().cpu().numpy(), ref_out.numpy())
    print(f"[wide mesh {tag} {device}] forward vs oracle {e:.2e}, loss {loss.item():.6f} vs {ref_loss.item():.6f}")
    assert e < 1e-5
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    masks = ou.engine_relu_masks(eng)
    assert set(masks) == {("backcast", l) for l in range(kw["n_layers"])}
    named = dict(blk.named_parameters())
    assert set(eng.param_names) == set(named)
    ou.check_grads_at_rounding_level(f"wide mesh {tag} {device}", {n: named[n].grad.cpu().numpy() for n in eng.param_names},
                                     lambda dt: oracle_run(kw, seed, B, S, padding, dt, masks)[2])
    ex = rel_l2(x.grad.cpu().numpy(), oracle_run(kw, seed, B, S, padding, relu_masks=masks)[3])
    print(f"[wide mesh {tag} {device}] dL/dx vs oracle {ex:.2e}")
    assert tuple(x.grad.shape) == x_np.shape and ex < 5e-5


@pytest.mark.parametrize("tag", ["2d_w96_unshared_f4", "2d_w128_shared_f2", "3d_w96_unshared_pad2"])
def test_wide_mesh_forward_and_every_gradient_vs_oracle(host_device, tag):
    """Forward < 1e-5, loss within 1e-5; every parameter gradient (oracle_util.check_grads_at_rounding_level) and the input
    gradient < 5e-5 against the oracle evaluated on the engine's own ReLU active sets."""
    check_forward_and_every_gradient(tag, host_device)


@pytest.mark.gpu
def test_wide_mesh3d_width128_real_padding_on_gpu():
    """The padding the model ships with (8): 5 x 3 x 4 -> 13 x 11 x 12, shared Fourier weights (their gradients folded over the
    layers), width 128.  Too slow for the emulator, so on the MI355X only."""
    check_forward_and_every_gradient("3d_w128_shared_pad8", "cuda:0")


@pytest.mark.parametrize("name", ["mesh2d_w96", "mesh3d_w96"])
def test_wide_mesh_vs_reference_golden(host_device, name):
    """tests/golden/mesh{2,3}d_w96.npz come from the imported reference itself (tools/make_golden.py), at its padding of 8:
    forward and loss."""
    g = gu.load_golden(name)
    kw = gu.golden_kwargs(g)
    meta = [int(v) for v in g["meta"]]
    B, S, seed = meta[0], tuple(meta[1:-1]), meta[-1]
    assert kw["width"] == 96 and len(S) == _kind(kw)
    blk = build_model(kw, seed, host_device)
    x_np, t_np = make_io(kw, seed, B, S)
    with torch.no_grad():
        out = blk(torch.from_numpy(x_np).to(host_device))
    assert gu.compare_packed(g, "out", out.cpu().numpy(), 1e-5) < 1e-5
    loss = ((out - torch.from_numpy(t_np).to(host_device)) ** 2).mean()
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * max(1.0, float(g["loss"]))


def test_wide_mesh_padding_is_applied(host_device):
    """A forward with padding 8 is the oracle's with padding 8 and NOT the oracle's with padding 2: a pad the engine ignored or
    shortened would pass an engine-vs-engine comparison."""
    kw, seed, B, S, _ = CASES["2d_w96_unshared_f4"]
    blk = build_model(kw, seed, host_device, padding=8)
    x_np, _ = make_io(kw, seed, B, S)
    with torch.no_grad():
        pred = blk(torch.from_numpy(x_np).to(host_device)).cpu().numpy()
        sd, _ = ou.torch_state_dict(state_dict_np(kw, seed), requires_grad=False)
        ref8 = oracle_forward(kw, sd, torch.from_numpy(x_np), 8).numpy()
        ref2 = oracle_forward(kw, sd, torch.from_numpy(x_np), 2).numpy()
    assert rel_l2(pred, ref8) < 1e-5
    assert rel_l2(ref2, ref8) > 1e-3 and rel_l2(pred, ref2) > 1e-3


@pytest.mark.parametrize("tag", ["2d_w96_unshared_f4", "3d_w96_unshared_pad2"])
def test_wide_mesh_second_forward_after_a_backward_is_bit_identical(host_device, tag):
    """The padded layer input is a ping-pong buffer the layers overwrite, pad region included: the embed re-zeroes it on every
    pass.  A stale pad region would change the second forward."""
    kw, seed, _, S, padding = CASES[tag]
    blk = build_model(kw, seed, host_device, padding)
    x_np, t_np = make_io(kw, seed, 1, S)
    x, t = torch.from_numpy(x_np).to(host_device), torch.from_numpy(t_np).to(host_device)
    first = blk(x)
    orc.lp_rel_loss(first, t).backward()
    first = first.detach().clone()
    second = blk(x).detach()
    assert torch.equal(first, second)
    with torch.no_grad():      # ... and the inference pass (its own recording, one slot) agrees to the bit as well
        assert torch.equal(blk(x), first)


def test_wide_mesh_state_dict_is_the_reference_layout_and_round_trips():
    from fourierflow_amd.modules import FNOFactorizedMesh2D, FNOFactorizedMesh3D
    for kw in (M2_W96, M2_W128, M3_W96, M3_W128):
        cls = FNOFactorizedMesh3D if _kind(kw) == 3 else FNOFactorizedMesh2D
        blk = cls(**kw)
        ref = state_dict_np(kw, 0)
        assert set(blk.state_dict().keys()) == set(ref.keys())      # (with share_weight: the duplicated per-layer keys too)
        for name, v in blk.state_dict().items():
            assert tuple(v.shape) == ref[name].shape, name
        buf = io.BytesIO()
        torch.save(blk.state_dict(), buf)
        buf.seek(0)
        other = cls(**kw)
        other.load_state_dict(torch.load(buf), strict=True)
        for (n, a), (_, b) in zip(blk.state_dict().items(), other.state_dict().items()):
            assert torch.equal(a, b), n


def test_wide_mesh_refusals_name_the_option(monkeypatch):
    from fourierflow_amd.modules import FNOFactorizedMesh2D, FNOFactorizedMesh3D
    for cls, base in ((FNOFactorizedMesh2D, M2_W96), (FNOFactorizedMesh3D, M3_W96)):
        for bad, word in ((dict(layer_norm=True), "layer_norm"), (dict(n_ff_layers=3), "n_ff_layers")):
            with pytest.raises(NotImplementedError, match=word) as ei:
                cls(**{**base, **bad}).engine()
            assert "32 / 64" in str(ei.value)
        with pytest.raises(NotImplementedError, match="factor"):
            cls(**{**base, "width": 256, "factor": 8}).engine()
        # the mode bound is on the PADDED length: 13 // 2 = 6 modes fit the 5 + 8 axis, 7 do not; more than 64 never do
        with pytest.raises(ValueError, match="modes"):
            cls(**{**base, "modes_x": 65}).engine()
    monkeypatch.setenv("FFNO_STORAGE", "bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        FNOFactorizedMesh2D(**M2_W96).engine()


def test_wide_mesh_mode_bound_is_on_the_padded_length(host_device):
    kw, seed, B, S, _ = CASES["2d_w96_unshared_f4"]
    x = torch.from_numpy(make_io(kw, seed, B, S)[0]).to(host_device)
    with torch.no_grad():
        assert tuple(build_model({**kw, "modes_x": 6}, seed, host_device)(x).shape) == (B, *S, 1)      # 6 == (5 + 8) // 2
        with pytest.raises(ValueError, match="modes"):
            build_model({**kw, "modes_x": 7}, seed, host_device)(x)


def test_narrow_mesh_widths_behave_as_before():
    from fourierflow_amd.engine import FFNOEngine
    from fourierflow_amd.modules import CNOFactorizedMesh2D, FNOFactorizedMesh2D, FNOFactorizedMesh3D
    for cls, base in ((FNOFactorizedMesh2D, M2_W96), (FNOFactorizedMesh3D, M3_W96)):
        assert type(cls(**{**base, "width": 64}).engine()) is FFNOEngine
        with pytest.raises(ValueError, match="compiled HIP kernel set"):      # not a wide width either: the main engine's refusal
            cls(**{**base, "width": 48}).engine()
        with pytest.raises(ValueError, match="compiled HIP kernel set"):
            cls(**{**base, "width": 288}).engine()
    with pytest.raises(ValueError, match="compiled HIP kernel set"):          # the DCT operators stay at 32 / 64
        CNOFactorizedMesh2D(**M2_W96).engine()


def test_airfoil_width128_example_trains_tests_and_predicts_through_the_cli(tmp_path, host_device):
    """`python -m fourierflow_amd train | test | predict` on the example config (shrunk to two layers on a 5 x 4 mesh): an
    optimisation step, the checkpoint with the wide engine's flat buffers, the test metric and a prediction file."""
    import json
    import shutil

    from typer.testing import CliRunner

    from fourierflow_amd.cli import app
    cfg = tmp_path / "config.yaml"
    shutil.copy(os.path.join(ROOT, "examples", "airfoil_width128.yaml"), cfg)
    small = ["routine.model.n_layers=2", "routine.model.modes_x=3", "routine.model.modes_y=2", "routine.model.factor=2",
             "builder.batch_size=1"]

    def run(*args):
        res = CliRunner().invoke(app, [*args, *small, "--size", "5", "--size", "4", "--device", host_device])
        assert res.exit_code == 0, (res.output, res.exception)
        return [json.loads(l) for l in res.output.splitlines() if l.startswith("{")]

    out = run("train", str(cfg), "--steps", "1")
    assert out[0]["step"] == 0 and np.isfinite(out[0]["train_loss"]) and np.isfinite(out[-1]["valid_loss"])
    assert np.isfinite(run("test", str(cfg), "--batches", "1")[-1]["test_loss"])
    assert run("predict", str(cfg), "--batch-size", "1")[-1]["shape"] == [1, 5, 4, 1]


TRAIN_LOSS_TOL, TRAIN_PARAM_TOL = 2e-5, 2e-4      # the bars of test_wide_block.py


def test_wide_mesh_trainer_steps_match_adamw_on_oracle_gradients(host_device):
    """Three FFNOTrainer steps (fused AdamW + cosine warm-up on the flat buffers) of the 2-D width-96 model against the same three
    steps of torch.optim.AdamW x the cosine factor on the oracle's gradients."""
    from fourierflow_amd.trainer import FFNOTrainer
    kw, seed, _, S, padding = CASES["2d_w96_unshared_f4"]
    B = 1
    blk = build_model(kw, seed, host_device, padding)
    hp = dict(lr=2.5e-3, weight_decay=1e-4, num_warmup_steps=2, num_training_steps=10)
    tr = FFNOTrainer(blk, **hp)
    sd, uniq = ou.torch_state_dict(state_dict_np(kw, seed))
    opt = torch.optim.AdamW(list(uniq.values()), lr=hp["lr"], weight_decay=hp["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: orc.cosine_warmup_factor(s, 2, 10))
    x_np, t_np = make_io(kw, seed, B, S)
    x, t = torch.from_numpy(x_np).to(host_device), torch.from_numpy(t_np).to(host_device)
    for step in range(3):
        loss = tr.train_step(x, t)
        opt.zero_grad()
        ref_loss = orc.lp_rel_loss(oracle_forward(kw, sd, torch.tensor(x_np), padding), torch.tensor(t_np))
        ref_loss.backward()
        opt.step()
        sched.step()
        assert abs(loss.item() - ref_loss.item()) < TRAIN_LOSS_TOL * max(1.0, ref_loss.item()), step
    named = dict(blk.named_parameters())
    for n, p in uniq.items():
        assert rel_l2(named[n].detach().cpu().numpy(), p.detach().numpy()) < TRAIN_PARAM_TOL, n


def test_airfoil_width128_example_builds_and_its_first_step_is_the_oracle_loss(host_device):
    """examples/airfoil_width128.yaml is the airfoil geometry at width 128 on the wide mesh engine; shrunk by overrides, the
    routine's first training step returns the oracle's relative-L2 loss."""
    from fourierflow_amd.config import build_routine, load_config
    from fourierflow_amd.engine_wide import WideFFNOMeshEngine
    from fourierflow_amd.routines import StructuredMeshExperiment
    path = os.path.join(ROOT, "examples", "airfoil_width128.yaml")
    exp = build_routine(load_config(path))
    assert isinstance(exp, StructuredMeshExperiment)
    m = exp.model
    assert (m.width, m.n_layers, m.modes_x, m.modes_y, m.factor, m.padding) == (128, 4, 32, 16, 4, 8)
    eng = m.engine()
    assert isinstance(eng, WideFFNOMeshEngine) and (eng.C, eng.H, eng.L, eng.Ks, eng.pad) == (128, 512, 4, (32, 16), 8)

    exp = build_routine(load_config(path, ["routine.model.modes_x=3", "routine.model.modes_y=2", "routine.model.n_layers=2",
                                           "routine.model.factor=2"]))
    kw = dict(modes_x=3, modes_y=2, width=128, input_dim=4, n_layers=2, share_weight=False, factor=2, ff_weight_norm=True,
              n_ff_layers=2, layer_norm=False)
    seed, B, S = 45, 2, (5, 4)
    sd_np = state_dict_np(kw, seed)
    exp.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    exp = exp.to(host_device)
    x_np, t_np = make_io(kw, seed, B, S)
    sd, _ = ou.torch_state_dict(sd_np, requires_grad=False)
    ref = orc.lp_rel_loss(oracle_forward(kw, sd, torch.from_numpy(x_np), 8), torch.from_numpy(t_np))
    l0 = exp.training_step(dict(x=torch.from_numpy(x_np).to(host_device), y=torch.from_numpy(t_np).to(host_device))).item()
    assert isinstance(exp.trainer().engine, WideFFNOMeshEngine)
    assert abs(l0 - ref.item()) < 1e-5
