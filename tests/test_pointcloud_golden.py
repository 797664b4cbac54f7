"""The float64 restatement of tests/pointcloud_model_oracle.py is the reference: evaluated in fp32 on the reference's own
weights and inputs it reproduces the outputs (<= 1e-5) and parameter gradients (<= 5e-5) that the reference modules produced
(tests/golden/pointcloud_ref.npz, written by tools/make_golden_pointcloud.py from the real iphi.py / point_cloud_2d.py), and
the module mirrors have the reference's state-dict names, shapes and dtypes and load its weights with strict=True.  No GPU."""
import os

import numpy as np
import pytest
import torch

import pointcloud_model_oracle as pmo
from backend_util import rel_l2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointcloud_ref.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _weights(gold, tag, who):
    """The reference state dict of the tagged model: the shared one is the plain one with the shared Fourier weights."""
    names = gold[f"{tag}.{who}.names"].tolist()
    sd = {}
    for k in names:
        if f"{tag}.{who}.w.{k}" in gold:
            v = gold[f"{tag}.{who}.w.{k}"]
        elif "fourier_weight" in k:                       # convs.{i}.fourier_weight.{j} aliases fourier_weight.{j}
            v = gold[f"{tag}.{who}.w.fourier_weight.{k[-1]}"]
        else:
            v = gold[f"plain.{who}.w.{k}"]
        sd[k] = torch.tensor(v)
    return sd


def _mirrors(gold, share):
    from fourierflow_amd.modules import FNOFactorizedPointCloud2D, IPhi
    B, W, M1, M2, S1, S2, N, IW, L = gold["shape"].tolist()
    return FNOFactorizedPointCloud2D(M1, M2, W, 2, 1, n_layers=L, s1=S1, s2=S2, share_weight=share), IPhi(IW)


@pytest.mark.parametrize("tag,share", [("plain", False), ("shared", True)])
def test_state_dict_layout_and_strict_load(gold, tag, share):
    for who, mod in zip(("model", "iphi"), _mirrors(gold, share)):
        sd = mod.state_dict()
        assert list(sd.keys()) == gold[f"{tag}.{who}.names"].tolist()
        assert [",".join(map(str, v.shape)) for v in sd.values()] == gold[f"{tag}.{who}.shapes"].tolist()
        assert [str(v.dtype) for v in sd.values()] == gold[f"{tag}.{who}.dtypes"].tolist()
        mod.load_state_dict(_weights(gold, tag, who), strict=True)
        for k, v in mod.state_dict().items():
            assert torch.equal(v, _weights(gold, tag, who)[k]), k
    model, iphi = _mirrors(gold, share)
    assert not isinstance(iphi.center, torch.nn.Parameter) and "center" not in dict(iphi.named_buffers())
    assert "B" not in dict(iphi.named_buffers()) and tuple(iphi.B.shape) == (1, 1, 1, iphi.width // 4)


@pytest.mark.parametrize("tag,share", [("plain", False), ("shared", True)])
def test_restatement_reproduces_the_reference(gold, tag, share):
    B, W, M1, M2, S1, S2, N, IW, L = gold["shape"].tolist()
    model, iphi = _mirrors(gold, share)
    model.load_state_dict(_weights(gold, tag, "model"), strict=True)
    iphi.load_state_dict(_weights(gold, tag, "iphi"), strict=True)
    sd, uniq = pmo.model_state_dict(model.state_dict(), torch.float32)
    isd, iuniq = pmo.model_state_dict(iphi.state_dict(), torch.float32)
    out = pmo.model(sd, torch.tensor(gold["xy"]), torch.tensor(gold["rr"]), iphi_sd=isd, iphi_width=IW, modes1=M1, modes2=M2,
                    width=W, n_layers=L, s1=S1, s2=S2)
    e = rel_l2(out.detach().numpy(), gold[f"{tag}.out"])
    loss = pmo.rel_l2_loss(out, torch.tensor(gold["sigma"]))
    assert e <= 1e-5 and abs(float(loss.detach()) - float(gold[f"{tag}.loss"])) <= 2e-5
    loss.backward()
    worst, checked = 0.0, 0
    for who, leaves in (("model", uniq), ("iphi", iuniq)):
        for k, t in leaves.items():
            key = f"{tag}.{who}.g.{k}"
            if f"{tag}.{who}.nograd.{k}" in gold:
                assert t.grad is None, k              # ws.*, fc_no_code.*: the reference leaves .grad at None
                continue
            if key not in gold:                       # (the shared file keeps the Fourier-weight gradients only)
                assert tag == "shared"
                continue
            g = torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad
            err = rel_l2(g.numpy(), gold[key])
            worst, checked = max(worst, err), checked + 1
            assert err <= 5e-5, (k, err)
    assert checked >= (2 if share else 30)
    print(f"[{tag}] forward {e:.2e}, worst of {checked} gradients {worst:.2e}")
