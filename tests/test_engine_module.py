"""The plumbing between the six engine-backed modules and their host engines (modules/_engine_module.py): the parameter list
handed to the engine, the one autograd node (stale passes, input gradients, fused accumulation) and the inference path
without a node.  Every class runs at the smallest configuration its own test file builds for the emulator."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as gu
from backend_util import host_device  # noqa: F401

CLASSES = ["FNOFactorized2DBlock", "FNOFactorizedMesh2D", "FNOFactorizedMesh3D", "FNOMesh2D", "FNOMesh3D", "FNOZongyi2DBlock"]
FFNO_CLASSES = CLASSES[:3]            # FFNOEngine: the input gradient is eng.dx
GENERATION_CHECKED = CLASSES[:4]      # one workspace: only the latest pass can be back-propagated


def _load(blk, sd_np):
    blk.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return blk


def _build(name, device):
    """-> (module on ``device``, input tensor on ``device``)."""
    from fourierflow_amd import modules as M
    if name == "FNOFactorized2DBlock":
        torch.manual_seed(0)
        blk = M.FNOFactorized2DBlock(modes=4, width=64, input_dim=3, n_layers=1, factor=4)
        x = np.random.RandomState(1).standard_normal((1, 8, 10, 3)).astype(np.float32)
    elif name == "FNOFactorizedMesh2D":        # test_mesh2d.py::test_mesh2d_structured_mesh_routine
        kw = dict(modes_x=3, modes_y=2, width=32, input_dim=4, n_layers=2, share_weight=False, factor=4, ff_weight_norm=True,
                  n_ff_layers=2, layer_norm=False)
        blk = _load(M.FNOFactorizedMesh2D(**kw), gu.make_mesh2d_state_dict(kw, 11))
        x, _ = gu.make_mesh2d_io(kw, 11, 2, (6, 5))
    elif name == "FNOFactorizedMesh3D":
        g = gu.load_golden("mesh3d_c32_small")
        kw, meta = gu.golden_kwargs(g), [int(v) for v in g["meta"]]
        blk = _load(M.FNOFactorizedMesh3D(**kw), gu.make_mesh3d_state_dict(kw, meta[4]))
        x, _ = gu.make_mesh3d_io(kw, meta[4], meta[0], tuple(meta[1:4]))
    elif name in ("FNOMesh2D", "FNOMesh3D"):
        g = gu.load_golden("geofno_c32" if name == "FNOMesh2D" else "geofno_3d_c32")
        kw = gu.golden_kwargs(g)
        B, X, Y, seed, Z = [int(v) for v in g["meta"]]
        blk = _load(getattr(M, name)(**kw), gu.make_geofno_state_dict(kw, seed))
        x, _ = gu.make_geofno_io(seed, B, X, Y, Z)
    else:                                      # test_zongyi.py: width 20 inside the 32-channel tile, modes 3, two layers
        kw = dict(modes1=3, modes2=3, width=20, input_dim=12, n_layers=2)
        blk = _load(M.FNOZongyi2DBlock(**kw), gu.make_zongyi_state_dict(kw, 5)[0])
        x = np.random.RandomState(6).standard_normal((2, 12, 12, 12)).astype(np.float32)
    return blk.to(device), torch.from_numpy(x).to(device)


def _out(res):
    return res["forecast"] if isinstance(res, dict) else res


@pytest.mark.parametrize("name", CLASSES)
def test_engine_parameters_follow_the_engine_order_and_see_a_replaced_parameter(host_device, name):
    blk, _ = _build(name, host_device)
    named = dict(blk.named_parameters())
    got = blk.engine_parameters()
    assert [n for n, _ in got] == list(blk.engine().param_names)
    assert all(isinstance(p, nn.Parameter) and p is named[n] for n, p in got)
    assert all(a is b for (_, a), (_, b) in zip(got, blk.engine_parameters()))
    victim = blk.engine().param_names[len(got) // 2]
    owner, _, attr = victim.rpartition(".")
    new = nn.Parameter(named[victim].detach().clone())
    setattr(blk.get_submodule(owner), attr, new)
    again = dict(blk.engine_parameters())
    assert again[victim] is new
    assert all(again[n] is named[n] for n in named if n != victim and n in again)


@pytest.mark.parametrize("name", GENERATION_CHECKED)
def test_only_the_most_recent_forward_can_be_back_propagated(host_device, name):
    blk, x = _build(name, host_device)
    first = _out(blk(x))
    _out(blk(x))
    with pytest.raises(RuntimeError, match="most recent forward"):
        first.sum().backward()


def test_geofno_input_gradient_is_refused_at_backward(host_device):
    blk, x = _build("FNOMesh2D", host_device)
    out = blk(x.requires_grad_(True))
    with pytest.raises(RuntimeError, match="INPUT"):
        out.sum().backward()


@pytest.mark.parametrize("name", FFNO_CLASSES)
def test_input_gradient_is_the_engines_dx(host_device, name):
    blk, x = _build(name, host_device)
    xg = x.clone().requires_grad_(True)
    out = _out(blk(xg))
    gy = torch.from_numpy(np.random.RandomState(2).standard_normal(tuple(out.shape)).astype(np.float32)).to(host_device)
    out.backward(gy)
    assert xg.grad is not None and tuple(xg.grad.shape) == tuple(x.shape)
    assert float(xg.grad.abs().max()) > 0.0
    eng = blk.engine()
    eng.forward(blk.prepare_input(x), True, training=blk.training)
    eng.backward(gy, need_dx=True)
    # (the meshes append their grid channels in prepare_input: the module's input gradient is the leading channels of dx)
    assert torch.equal(xg.grad, eng.dx[..., :x.shape[-1]])


@pytest.mark.parametrize("name", CLASSES)
def test_no_grad_forward_builds_no_node_and_training_still_works_after_it(host_device, name):
    blk, x = _build(name, host_device)
    with torch.no_grad():
        quiet = _out(blk(x))
    assert quiet.grad_fn is None and not quiet.requires_grad
    out = _out(blk(x))
    assert out.grad_fn is not None and tuple(out.shape) == tuple(quiet.shape)
    (out ** 2).mean().backward()
    for n, p in blk.engine_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape) and bool(torch.isfinite(p.grad).all()), n
    assert any(float(p.grad.abs().max()) > 0.0 for _, p in blk.engine_parameters())


def test_zongyi_fused_grad_accumulation_leaves_grad_none_and_fills_gflat(host_device):
    blk, x = _build("FNOZongyi2DBlock", host_device)
    blk.fused_grad_accumulation = True
    out = blk(x)["forecast"]
    blk.engine().zero_grad()
    (out ** 2).mean().backward()
    assert all(p.grad is None for p in blk.parameters())
    assert float(blk.engine().gflat.abs().max()) > 0.0
