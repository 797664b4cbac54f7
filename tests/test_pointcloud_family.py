"""What the three point-cloud models share (modules/_point_cloud.py): one ``iphi`` evaluation on shared points, the latent grid's
values, passes that repeat themselves bit for bit, parameters that are re-read on every pass, the refusals of the forward
preface and the parameters kept out of the optimiser.  Every class runs at one small shape: N = 70 points is one full chunk of
the 64 the kernels walk at a time and a ragged one.  What each model computes is pinned by its own test files."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from backend_util import host_device  # noqa: F401

CLASSES = ["FNOFactorizedPointCloud2D", "FNOPointCloud2D", "FNOFullyFactorizedMesh2D"]
IPHI_OPTIONAL = CLASSES[:2]
B, N, W, M1, M2, S, L, IPHI_W = 2, 70, 32, 3, 2, 8, 2, 16
UNUSED = {"FNOFactorizedPointCloud2D": ("ws.",), "FNOPointCloud2D": (), "FNOFullyFactorizedMesh2D": ("ws.", f"convs.{L}.backcast_ff.")}


def _build(name, device="cpu", seed=0, **kw):
    """-> (model, IPhi) on ``device``."""
    from fourierflow_amd import modules as M
    torch.manual_seed(seed)
    model = getattr(M, name)(M1, M2, W, 2, 1, n_layers=L, s1=S, s2=S, **kw)
    return model.to(device), M.IPhi(IPHI_W).to(device)


def _io(device, seed=1, n=N):
    rng = np.random.default_rng(seed)
    put = lambda a: torch.tensor(a.astype(np.float32), device=device)      # noqa: E731
    return put(rng.uniform(0.05, 0.95, (B, n, 2))), put(rng.standard_normal((B, 42))), put(rng.standard_normal((B, n, 1)))


def _last_weights(model):
    last = model.convs[-1]
    return list(last.fourier_weight) if hasattr(last, "fourier_weight") else [last.weights1, last.weights2]


def _pass(model, iphi, xy, rr, gy):
    """One forward and backward from zeroed gradients -> (output, {name: gradient})."""
    model.zero_grad(set_to_none=True), iphi.zero_grad(set_to_none=True)
    out = model(xy, code=rr, iphi=iphi)
    out.backward(gy)
    grads = {who + k: p.grad.clone() for who, mod in (("model.", model), ("iphi.", iphi)) for k, p in mod.named_parameters()
             if p.grad is not None}
    return out.detach().clone(), grads


@pytest.mark.parametrize("name", CLASSES)
def test_iphi_runs_once_on_shared_points(host_device, name):
    model, iphi = _build(name, host_device)
    calls = []
    handle = iphi.register_forward_hook(lambda *a: calls.append(1))
    xy, rr, _ = _io(host_device)
    with torch.no_grad():
        model(xy, code=rr, iphi=iphi)
        assert len(calls) == 1
        model(xy, code=rr, x_in=xy, x_out=xy, iphi=iphi)
        assert len(calls) == 2
        model(xy, code=rr, x_in=xy, x_out=xy.clone(), iphi=iphi)      # equal values, another tensor: two evaluations
        assert len(calls) == 4
    handle.remove()


@pytest.mark.parametrize("name", CLASSES)
def test_get_grid_is_the_references_linspace(host_device, name):
    model, _ = _build(name)
    grid = model.get_grid([2, 8, 9], host_device)
    assert tuple(grid.shape) == (2, 8, 9, 2) and grid.dtype == torch.float32 and grid.device == torch.device(host_device)
    gx = torch.tensor(np.linspace(0, 1, 8), dtype=torch.float).reshape(1, 8, 1, 1).repeat([2, 1, 9, 1])
    gy = torch.tensor(np.linspace(0, 1, 9), dtype=torch.float).reshape(1, 1, 9, 1).repeat([2, 8, 1, 1])
    assert torch.equal(grid.cpu(), torch.cat((gx, gy), dim=-1))


@pytest.mark.parametrize("name", CLASSES)
def test_two_passes_on_the_same_inputs_are_bit_identical(host_device, name):
    model, iphi = _build(name, host_device)
    xy, rr, gy = _io(host_device)
    out1, g1 = _pass(model, iphi, xy, rr, gy)
    out2, g2 = _pass(model, iphi, xy, rr, gy)
    assert torch.equal(out1, out2)
    assert list(g1) == list(g2) and len(g1) > 0
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert all(not k.startswith(tuple("model." + p for p in UNUSED[name]) + ("iphi.fc_no_code.",)) for k in g1)


@pytest.mark.parametrize("name", CLASSES)
def test_a_replaced_parameter_is_seen_by_the_next_pass(host_device, name):
    model, iphi = _build(name, host_device)
    xy, rr, gy = _io(host_device)
    before, _ = _pass(model, iphi, xy, rr, gy)      # whatever is kept across passes is now filled
    model.fc0.weight = nn.Parameter(model.fc0.weight.detach() * 1.25 + 0.01)
    model.bs[0].weight = nn.Parameter(model.bs[0].weight.detach() * 0.75 - 0.02)
    with torch.no_grad():
        for w in _last_weights(model):
            w.mul_(1.5)
    fresh, _ = _build(name, host_device, seed=5)
    fresh.load_state_dict(model.state_dict(), strict=True)
    out, grads = _pass(model, iphi, xy, rr, gy)
    ref, ref_grads = _pass(fresh, iphi, xy, rr, gy)
    assert not torch.equal(out, before)
    assert torch.equal(out, ref)
    assert list(grads) == list(ref_grads)
    for k in grads:
        assert torch.equal(grads[k], ref_grads[k]), k


@pytest.mark.parametrize("name", CLASSES)
def test_the_forward_preface_refuses(host_device, name):
    xy, rr, _ = _io(host_device)
    model, iphi = _build(name, host_device)
    with pytest.raises(ValueError):
        model(torch.zeros(B, N, 3, device=host_device), code=rr, iphi=iphi)
    loose, _ = _build(name, host_device, is_mesh=False)
    with pytest.raises(ValueError, match="x_in and x_out"):
        loose(xy, code=rr, iphi=iphi)
    with pytest.raises(ValueError, match="x_in and x_out"):
        loose(xy, code=rr, x_in=xy, iphi=iphi)
    if name in IPHI_OPTIONAL:
        with torch.no_grad():
            assert tuple(model(xy).shape) == (B, N, 1)
    else:
        with pytest.raises(ValueError, match="iphi"):
            model(xy, code=rr)


@pytest.mark.parametrize("name", CLASSES)
def test_cpu_tensors_raise_without_the_test_backend(name):
    from fourierflow_amd import _lib
    model, iphi = _build(name)
    with pytest.raises(_lib.FFNOLibraryError):
        model(torch.zeros(B, N, 2), code=torch.zeros(B, 42), iphi=iphi)        # HIP only


@pytest.mark.parametrize("name", CLASSES)
def test_unused_parameters_stay_out_of_the_optimiser(name):
    from fourierflow_amd.routines import PointCloudExperiment
    from fourierflow_amd.routines.point_cloud import _TrainedParameters
    model, iphi = _build(name)
    assert tuple(model.unused_parameter_prefixes) == UNUSED[name]
    routine = PointCloudExperiment(model, iphi, 10)
    skip = tuple("model." + p for p in UNUSED[name]) + ("iphi.fc_no_code.",)
    everything = [n for n, _ in routine.named_parameters()]
    assert [n for n, _ in _TrainedParameters(routine).engine_parameters()] == [n for n in everything if not n.startswith(skip)]
    left_out = [n for n in everything if n.startswith(skip)]
    assert len(left_out) == 2 + {"FNOFactorizedPointCloud2D": 2 * (L - 1), "FNOPointCloud2D": 0,
                                 "FNOFullyFactorizedMesh2D": 2 * (L - 1) + 6}[name]
