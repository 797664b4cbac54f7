"""FNOFactorized2DBlock at widths 96 / 128: the GEMM-composed wide engine (fourierflow_amd/engine_wide.py over csrc/bgemm.hip)
against the oracle, the reference's golden vectors, its state-dict layout and an AdamW run -- on the CPU wave emulator
(-m "not gpu") and on the MI355X (-m gpu).  The method is that of test_block.py."""
import io

import numpy as np
import pytest
import torch

import golden_util as gu
import oracle_util as ou
from backend_util import host_device, rel_l2  # noqa: F401
from oracle import ffno_oracle as orc

W96 = dict(modes=3, width=96, n_layers=2, factor=4, input_dim=3, share_weight=True, ff_weight_norm=True, gain=0.1)
W128 = dict(modes=3, width=128, n_layers=2, factor=2, input_dim=5, share_weight=False, ff_weight_norm=True, gain=0.1)


def build_block(kw, seed, device):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    blk = FNOFactorized2DBlock(**kw)
    sd = {k: torch.from_numpy(v.copy()) for k, v in gu.make_block_state_dict(kw, seed).items()}
    blk.load_state_dict(sd, strict=True)
    return blk.to(device)


@pytest.mark.parametrize("kw,shape,seed", [(W96, (2, 10, 12), 21), (W128, (3, 8, 8), 22)], ids=["w96_shared_f4", "w128_unshared_f2"])
def test_wide_block_forward_and_every_gradient_vs_oracle(host_device, kw, shape, seed):
    """Forward < 1e-5; every parameter gradient and the input gradient < 5e-5 against the oracle evaluated on the engine's own
    ReLU active sets (heavily cancelling sums -- the head biases -- against the fp64 oracle within 4x the fp32 oracle's own
    noise: oracle_util.check_grads_at_rounding_level)."""
    from fourierflow_amd.engine_wide import WideFFNO2DEngine
    B, M, N = shape
    blk = build_block(kw, seed, host_device)
    eng = blk.engine()
    assert isinstance(eng, WideFFNO2DEngine)
    x_np, t_np = gu.make_block_io(kw, seed, B, M, N)
    x = torch.from_numpy(x_np).to(host_device).requires_grad_(True)
    out = blk(x)
    assert out["forecast_list"] == []
    pred = out["forecast"]
    loss = orc.lp_rel_loss(pred, torch.from_numpy(t_np).to(host_device))
    loss.backward()
    ref_out, ref_loss, _ = ou.oracle_block_run(kw, seed, B, M, N)
    e = rel_l2(pred.detach().cpu().numpy(), ref_out["forecast"].detach().numpy())
    print(f"[wide block {kw['width']} {host_device}] forward vs oracle {e:.2e}")
    assert e < 1e-5
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    masks = ou.engine_relu_masks(eng)
    assert set(masks) == {("backcast", l) for l in range(kw["n_layers"])}
    named = dict(blk.named_parameters())
    assert set(eng.param_names) == set(named)
    ou.check_grads_at_rounding_level(f"wide block {kw['width']} {host_device}", {n: named[n].grad.cpu().numpy() for n in eng.param_names},
                                     lambda dt: ou.oracle_block_run(kw, seed, B, M, N, dtype=dt, relu_masks=masks)[2])
    # input gradient, on the same active sets
    sd, _ = ou.torch_state_dict(gu.make_block_state_dict(kw, seed))
    xo = torch.tensor(x_np, requires_grad=True)
    o = orc.ffno2d_block(sd, xo, modes=kw["modes"], n_layers=kw["n_layers"], relu_masks=masks)
    orc.lp_rel_loss(o["forecast"], torch.tensor(t_np)).backward()
    ex = rel_l2(x.grad.cpu().numpy(), xo.grad.numpy())
    print(f"[wide block {kw['width']} {host_device}] dL/dx vs oracle {ex:.2e}")
    assert tuple(x.grad.shape) == x_np.shape and ex < 5e-5


def test_wide_block_vs_reference_golden(host_device):
    """tests/golden/block_w96_2l.npz comes from the imported reference itself (tools/make_golden.py): forward and loss."""
    g = gu.load_golden("block_w96_2l")
    kw = gu.golden_kwargs(g)
    B, M, N, seed = [int(v) for v in g["meta"]]
    assert kw["width"] == 96
    blk = build_block(kw, seed, host_device)
    x_np, t_np = gu.make_block_io(kw, seed, B, M, N)
    with torch.no_grad():
        pred = blk(torch.from_numpy(x_np).to(host_device))["forecast"]
    assert gu.compare_packed(g, "forecast", pred.cpu().numpy(), 1e-5) < 1e-5
    loss = orc.lp_rel_loss(pred, torch.from_numpy(t_np).to(host_device))
    assert abs(loss.item() - float(g["loss"])) < 1e-5


def test_wide_state_dict_is_the_reference_layout_and_round_trips():
    from fourierflow_amd.modules import FNOFactorized2DBlock
    for kw in (W96, W128, {**W128, "ff_weight_norm": False}):
        blk = FNOFactorized2DBlock(**kw)
        ref = gu.make_block_state_dict(kw, 0)
        assert set(blk.state_dict().keys()) == set(ref.keys())      # (with share_weight: the duplicated per-layer keys too)
        for name, v in blk.state_dict().items():
            assert tuple(v.shape) == ref[name].shape, name
        buf = io.BytesIO()
        torch.save(blk.state_dict(), buf)
        buf.seek(0)
        other = FNOFactorized2DBlock(**kw)
        other.load_state_dict(torch.load(buf), strict=True)
        for (n, a), (_, b) in zip(blk.state_dict().items(), other.state_dict().items()):
            assert torch.equal(a, b), n


def test_wide_trainer_steps_match_adamw_on_oracle_gradients(host_device):
    """Three FFNOTrainer steps (fused AdamW + cosine warm-up on the flat buffers) at width 96 against the same three steps of
    torch.optim.AdamW x the cosine factor on the oracle's gradients.  The bar is that of
    test_trainer.py::test_train_steps_match_reference_golden (the width-64 training-step test)."""
    from fourierflow_amd.trainer import FFNOTrainer
    kw, seed, (B, M, N) = W96, 31, (1, 8, 8)
    blk = build_block(kw, seed, host_device)
    hp = dict(lr=2.5e-3, weight_decay=1e-4, num_warmup_steps=2, num_training_steps=10)
    tr = FFNOTrainer(blk, **hp)
    sd, uniq = ou.torch_state_dict(gu.make_block_state_dict(kw, seed))
    opt = torch.optim.AdamW(list(uniq.values()), lr=hp["lr"], weight_decay=hp["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: orc.cosine_warmup_factor(s, 2, 10))
    x_np, t_np = gu.make_block_io(kw, seed, B, M, N)
    x, t = torch.from_numpy(x_np).to(host_device), torch.from_numpy(t_np).to(host_device)
    for step in range(3):
        loss = tr.train_step(x, t)
        opt.zero_grad()
        out = orc.ffno2d_block(sd, torch.tensor(x_np), modes=kw["modes"], n_layers=kw["n_layers"])
        ref_loss = orc.lp_rel_loss(out["forecast"], torch.tensor(t_np))
        ref_loss.backward()
        opt.step()
        sched.step()
        assert abs(loss.item() - ref_loss.item()) < TRAIN_LOSS_TOL * max(1.0, ref_loss.item()), step
    named = dict(blk.named_parameters())
    for n, p in uniq.items():
        assert rel_l2(named[n].detach().cpu().numpy(), p.detach().numpy()) < TRAIN_PARAM_TOL, n


TRAIN_LOSS_TOL, TRAIN_PARAM_TOL = 2e-5, 2e-4


def test_wide_refusals_name_the_option():
    from fourierflow_amd.engine import FFNO2DEngine
    from fourierflow_amd.modules import FNOFactorized2DBlock
    base = dict(modes=3, width=96, input_dim=3, n_layers=2, factor=4)
    for bad, word in ((dict(use_fork=True), "use_fork"), (dict(layer_norm=True), "layer_norm"), (dict(dropout=0.1), "dropout"),
                      (dict(in_dropout=0.1), "dropout"), (dict(mode="low-pass"), "low-pass"), (dict(mode="no-fourier"), "no-fourier"),
                      (dict(n_ff_layers=3), "n_ff_layers"), (dict(share_fork=True), "share_fork")):
        with pytest.raises(NotImplementedError, match=word) as ei:
            FNOFactorized2DBlock(**{**base, **bad}).engine()
        assert "32 / 64" in str(ei.value)
    with pytest.raises(NotImplementedError, match="factor"):
        FNOFactorized2DBlock(**{**base, "width": 256, "factor": 8}).engine()
    with pytest.raises(ValueError, match="compiled HIP kernel set"):      # not a wide width either: the main engine's refusal
        FNOFactorized2DBlock(**{**base, "width": 48}).engine()
    assert type(FNOFactorized2DBlock(**{**base, "width": 64}).engine()) is FFNO2DEngine


def test_wide_refuses_bf16_storage(monkeypatch):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    monkeypatch.setenv("FFNO_STORAGE", "bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        FNOFactorized2DBlock(modes=3, width=96, input_dim=3, n_layers=2, factor=4).engine()
