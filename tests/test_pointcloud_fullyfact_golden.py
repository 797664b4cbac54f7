"""FNOFullyFactorizedMesh2D against the reference's own numbers (tests/golden/pointcloud_fullyfact_ref.npz, written by
tools/make_golden_pointcloud_fullyfact.py from the real reference modules), on the CPU alone: the state-dict layout is the
reference's, its state dict loads with strict=True, and the separable restatement of tests/pointcloud_fullyfact_oracle.py
reproduces the reference's fp32 output, loss and every gradient -- float64 against fp32, so the distance is the reference's own
rounding (forward 1.6e-7 .. 1.7e-6 over the shapes it was checked at; the bands here are 1e-5 forward and 5e-5 per gradient,
the project's standing ones).  The parameters the reference never reads have no gradient in either."""
import os

import numpy as np
import pytest
import torch

import pointcloud_fullyfact_oracle as pfo
import pointcloud_model_oracle as pmo
from backend_util import rel_l2

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointcloud_fullyfact_ref.npz"))
B, W, M1, M2, S, N, IPHI_W, N_LAYERS = (int(v) for v in GOLD["shape"])
CFG = dict(modes1=M1, modes2=M2, width=W, s=S)
FWD_TOL, GRAD_TOL = 1e-5, 5e-5


def golden_sd(who):
    return {k[len(who) + 3:]: torch.tensor(GOLD[k]) for k in GOLD.files if k.startswith(who + ".w.")}


def build(n_layers=N_LAYERS, seed=0, iphi_w=IPHI_W, **kw):
    from fourierflow_amd.modules import FNOFullyFactorizedMesh2D, IPhi
    torch.manual_seed(seed)
    cfg = dict(CFG, **kw)
    s = cfg.pop("s")
    model = FNOFullyFactorizedMesh2D(cfg.pop("modes1"), cfg.pop("modes2"), cfg.pop("width"), 2, 1, n_layers=n_layers, s1=s, s2=s, **cfg)
    return model, IPhi(iphi_w)


def oracle(model, iphi, xy, rr, sigma, dtype, cfg, n_layers, grads=True, x_out=None, pre_trace=None):
    """The restatement on a model's weights: output alone, or (output, loss, {name: gradient or None})."""
    sd, uniq = pmo.model_state_dict(model.state_dict(), dtype)
    isd, iuniq = pmo.model_state_dict(iphi.state_dict(), dtype)
    u = torch.tensor(xy, dtype=dtype)
    kw = {} if x_out is None else dict(x_in=u, x_out=torch.tensor(x_out, dtype=dtype))
    out = pfo.model(sd, u, torch.tensor(rr, dtype=dtype), n_layers=n_layers, iphi_sd=isd, iphi_width=iphi.width,
                    pre_trace=pre_trace, **{k: v for k, v in cfg.items() if k in ("modes1", "modes2", "width", "s")}, **kw)
    if not grads:
        return out.detach().numpy()
    loss = pmo.rel_l2_loss(out, torch.tensor(sigma, dtype=dtype))
    loss.backward()
    res = {"model." + k: None if v.grad is None else v.grad.numpy() for k, v in uniq.items()}
    res.update({"iphi." + k: None if v.grad is None else v.grad.numpy() for k, v in iuniq.items()})
    return out.detach().numpy(), float(loss.detach()), res


@pytest.mark.parametrize("n_layers", [int(v) for v in GOLD["layout_layers"]])
def test_state_dict_layout_is_the_references(n_layers):
    model, iphi = build(n_layers)
    sd = model.state_dict()
    assert list(sd.keys()) == list(GOLD[f"layout{n_layers}.names"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(GOLD[f"layout{n_layers}.shapes"])
    assert [str(v.dtype) for v in sd.values()] == list(GOLD[f"layout{n_layers}.dtypes"])
    assert sum(k.startswith("convs.") for k in sd) == 8 * (n_layers + 1) and sum(k.startswith("ws.") for k in sd) == 2 * (n_layers - 1)
    assert list(iphi.state_dict().keys()) == list(GOLD["iphi.names"])
    assert model.unused_parameter_prefixes == ("ws.", f"convs.{n_layers}.backcast_ff.")
    from fourierflow_amd.modules.factorized_fno import FNOFullyFactorizedMesh2D
    from fourierflow_amd.modules.factorized_fno.mesh_plus_2d import SpectralConv2d
    assert type(model) is FNOFullyFactorizedMesh2D and all(type(c) is SpectralConv2d for c in model.convs)


def test_reference_state_dict_loads_strict():
    model, iphi = build()
    ref = golden_sd("model")
    assert ref["convs.0.fourier_weight.0"].shape == (W, W, M2, 2) and ref["convs.0.fourier_weight.1"].shape == (W, W, M1, 2)
    model.load_state_dict(ref, strict=True)
    iphi.load_state_dict(golden_sd("iphi"), strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_restatement_reproduces_the_reference():
    model, iphi = build()
    model.load_state_dict(golden_sd("model")), iphi.load_state_dict(golden_sd("iphi"))
    out, loss, grads = oracle(model, iphi, GOLD["xy"], GOLD["rr"], GOLD["sigma"], torch.float64, CFG, N_LAYERS)
    e = rel_l2(GOLD["out"], out)
    print(f"reference fp32 vs float64 restatement: forward {e:.2e}, loss {abs(loss - float(GOLD['loss'])):.2e}")
    assert e < FWD_TOL
    assert abs(loss - float(GOLD["loss"])) < FWD_TOL * abs(float(GOLD["loss"]))
    n = worst = 0
    for who, mod in (("model", model), ("iphi", iphi)):
        for k, _ in mod.named_parameters():
            g = grads[f"{who}.{k}"]
            if f"{who}.nograd.{k}" in GOLD.files:
                assert g is None, k
                assert k.startswith(("ws.", f"convs.{N_LAYERS}.backcast_ff.", "fc_no_code.")), k
                continue
            e = rel_l2(GOLD[f"{who}.g.{k}"], g)
            worst = max(worst, e)
            assert e < GRAD_TOL, (who, k, e)
            n += 1
    print(f"worst gradient of the reference vs the restatement: {worst:.2e} over {n} parameters")
    # all but ws.0.{weight, bias}, the six of convs.L.backcast_ff and iphi.fc_no_code.{weight, bias}
    assert n == len(list(model.parameters())) + len(list(iphi.parameters())) - 10
