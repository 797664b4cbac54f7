"""FNOPointCloud2D (the geo-FNO elasticity baseline) + IPhi: state-dict layout and strict load against the reference's own
(tests/golden/pointcloud_geofno_ref.npz, written by tools/make_golden_pointcloud_geofno.py from the real reference modules),
ops.mix_corner_modes against the float64 einsum, and the model against BOTH the reference's own fp32 numbers and the float64
restatement of tests/pointcloud_geofno_oracle.py: forward <= 1e-5 rel-L2, every parameter gradient of model and IPhi <= 5e-5
(the project's standing bands; the reference's own fp32 rounding at this shape is 1.8e-7 / 7.9e-7).  On the emulator and on an
MI355X."""
import os

import numpy as np
import pytest
import torch

import pointcloud_geofno_oracle as pgo
import pointcloud_model_oracle as pmo
from backend_util import host_device, rel_l2  # noqa: F401  (host_device is a fixture)

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointcloud_geofno_ref.npz"))
B, W, M1, M2, S1, S2, N, IPHI_W, N_LAYERS = (int(v) for v in GOLD["shape"])
CFG = dict(modes1=M1, modes2=M2, width=W, s1=S1, s2=S2)
FWD_TOL, GRAD_TOL = 1e-5, 5e-5


def _golden_sd(who):
    return {k[len(who) + 3:]: torch.tensor(GOLD[k]) for k in GOLD.files if k.startswith(who + ".w.")}


def _build(n_layers=N_LAYERS, seed=0, iphi_w=IPHI_W, **kw):
    from fourierflow_amd.modules import FNOPointCloud2D, IPhi
    torch.manual_seed(seed)
    cfg = dict(CFG, **kw)      # (is_mesh goes along when given; the default is the constructor's)
    model = FNOPointCloud2D(cfg.pop("modes1"), cfg.pop("modes2"), cfg.pop("width"), 2, 1, n_layers=n_layers, **cfg)
    return model, IPhi(iphi_w)


def _io(n, seed, b=B):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.05, 0.95, (b, n, 2)).astype(np.float32), rng.standard_normal((b, 42)).astype(np.float32),
            rng.standard_normal((b, n, 1)).astype(np.float32))


def _oracle(model, iphi, xy, rr, sigma, dtype, cfg, n_layers, grads=True, x_out=None):
    sd, uniq = pmo.model_state_dict(model.state_dict(), dtype)
    kw = {}
    iuniq = {}
    if iphi is not None:
        isd, iuniq = pmo.model_state_dict(iphi.state_dict(), dtype)
        kw = dict(iphi_sd=isd, iphi_width=iphi.width)
    u = torch.tensor(xy, dtype=dtype)
    if x_out is not None:
        kw.update(x_in=u, x_out=torch.tensor(x_out, dtype=dtype))
    out = pgo.model(sd, u, None if rr is None else torch.tensor(rr, dtype=dtype), n_layers=n_layers, **cfg, **kw)
    if not grads:
        return out.detach().numpy()
    loss = pmo.rel_l2_loss(out, torch.tensor(sigma, dtype=dtype))
    loss.backward()

    def g(t):
        if t.grad is None:
            return None
        return (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad).numpy()
    res = {"model." + k: g(v) for k, v in uniq.items()}
    res.update({"iphi." + k: g(v) for k, v in iuniq.items()})
    return out.detach().numpy(), float(loss.detach()), res


@pytest.mark.parametrize("n_layers", [int(v) for v in GOLD["layout_layers"]])
def test_state_dict_layout_is_the_references(n_layers):
    model, iphi = _build(n_layers)
    sd = model.state_dict()
    assert list(sd.keys()) == list(GOLD[f"layout{n_layers}.names"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(GOLD[f"layout{n_layers}.shapes"])
    assert [str(v.dtype) for v in sd.values()] == list(GOLD[f"layout{n_layers}.dtypes"])
    assert sum(k.startswith("convs.") for k in sd) == 2 * (n_layers + 1) and sum(k.startswith("ws.") for k in sd) == 2 * (n_layers - 1)
    assert list(iphi.state_dict().keys()) == list(GOLD["iphi.names"])
    from fourierflow_amd.modules.zongyi_fno import FNOPointCloud2D
    assert type(model) is FNOPointCloud2D


def test_reference_state_dict_loads_strict():
    model, iphi = _build()
    ref = _golden_sd("model")
    assert ref["convs.0.weights1"].dtype == torch.complex64
    model.load_state_dict(ref, strict=True)
    iphi.load_state_dict(_golden_sd("iphi"), strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref[k]), k


def test_mix_corner_modes_is_the_corner_einsum(host_device):
    from fourierflow_amd import ops
    rng = np.random.default_rng(1)
    cplx = lambda shape, scale=1.0: ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)  # noqa: E731
    V, w1, w2, g = cplx((B, W, 2 * M1, M2)), cplx((W, W, M1, M2), 1 / W), cplx((W, W, M1, M2), 1 / W), cplx((B, W, 2 * M1, M2))
    real = lambda a: torch.view_as_real(torch.tensor(a, device=host_device)).clone()  # noqa: E731
    z = real(V).permute(3, 2, 0, 4, 1).contiguous().requires_grad_(True)              # [m2, 2 m1, B, 2, C]
    w1t, w2t = real(w1).requires_grad_(True), real(w2).requires_grad_(True)
    for grid in (None, (S1, S2)):
        out = ops.mix_corner_modes(z, w1t, w2t, grid)
        assert out.shape == z.shape
        V64, a64, b64 = (torch.tensor(a.astype(np.complex128), requires_grad=True) for a in (V, w1, w2))
        ref = torch.cat([torch.einsum("bixy,ioxy->boxy", V64[:, :, :M1], a64),
                         torch.einsum("bixy,ioxy->boxy", V64[:, :, M1:], b64)], dim=-2)
        back = lambda t: t.permute(2, 4, 1, 0, 3).detach().cpu().numpy()              # noqa: E731  -> [B, C, 2 m1, m2, 2]
        assert rel_l2(back(out), torch.view_as_real(ref).detach().numpy()) < FWD_TOL
        dz, d1, d2 = torch.autograd.grad(out, (z, w1t, w2t), real(g).permute(3, 2, 0, 4, 1).contiguous())
        rz, r1, r2 = torch.autograd.grad(ref, (V64, a64, b64), torch.tensor(g.astype(np.complex128)))
        assert rel_l2(back(dz), torch.view_as_real(rz).numpy()) < GRAD_TOL
        assert rel_l2(d1.cpu().numpy(), torch.view_as_real(r1).numpy()) < GRAD_TOL
        assert rel_l2(d2.cpu().numpy(), torch.view_as_real(r2).numpy()) < GRAD_TOL
    with pytest.raises(ValueError):
        ops.mix_corner_modes(z, w1t[:, :, :2], w2t[:, :, :2])


_REF64 = {}


def _golden_oracle():
    """The float64 restatement on the golden's weights and inputs, computed once for the module."""
    if not _REF64:
        model, iphi = _build()
        model.load_state_dict(_golden_sd("model")), iphi.load_state_dict(_golden_sd("iphi"))
        _REF64["v"] = _oracle(model, iphi, GOLD["xy"], GOLD["rr"], GOLD["sigma"], torch.float64, CFG, N_LAYERS)
    return _REF64["v"]


def test_model_against_the_reference_and_the_float64_restatement(host_device):
    ref64, loss64, g64 = _golden_oracle()
    # the restatement is the reference's model: its distance from the reference's fp32 output is the reference's own rounding
    print(f"reference fp32 vs float64 restatement: forward {rel_l2(GOLD['out'], ref64):.2e}")
    assert rel_l2(GOLD["out"], ref64) < 2e-6
    model, iphi = _build()
    model.load_state_dict(_golden_sd("model")), iphi.load_state_dict(_golden_sd("iphi"))
    model.to(host_device), iphi.to(host_device)
    dev = lambda a: torch.tensor(np.asarray(a), device=host_device)      # noqa: E731
    out = model(dev(GOLD["xy"]), code=dev(GOLD["rr"]), iphi=iphi)
    assert out.shape == (B, N, 1)
    got = out.detach().cpu().numpy()
    e_ref, e64 = rel_l2(got, GOLD["out"]), rel_l2(got, ref64)
    print(f"forward vs reference fp32 {e_ref:.2e}, vs float64 {e64:.2e}")
    assert e_ref < FWD_TOL and e64 < FWD_TOL
    loss = pmo.rel_l2_loss(out, dev(GOLD["sigma"]))
    assert abs(loss.item() - float(GOLD["loss"])) < FWD_TOL * abs(float(GOLD["loss"]))
    loss.backward()
    n = 0
    for prefix, who, mod in (("model.", "model", model), ("iphi.", "iphi", iphi)):
        for k, p in mod.named_parameters():
            if f"{who}.nograd.{k}" in GOLD.files:
                assert p.grad is None and g64[prefix + k] is None, k
                assert k.startswith("fc_no_code.") and who == "iphi", k
                continue
            assert p.grad is not None, prefix + k
            g = p.grad.detach().cpu().numpy()
            e_ref, e64 = rel_l2(g, GOLD[f"{who}.g.{k}"]), rel_l2(g, g64[prefix + k])
            print(f"grad {prefix + k}: vs reference fp32 {e_ref:.2e}, vs float64 {e64:.2e}")
            assert e_ref < GRAD_TOL and e64 < GRAD_TOL, prefix + k
            n += 1
    assert n == len(list(model.parameters())) + len(list(iphi.parameters())) - 2      # all but iphi.fc_no_code.{weight, bias}


def test_one_layer_model(host_device):
    """n_layers = 1: no middle layer, ws empty; forward and every gradient against the float64 restatement."""
    model, iphi = _build(1, seed=3)
    assert len(model.ws) == 0 and len(model.convs) == 2 and len(model.bs) == 2
    xy, rr, sigma = _io(N, 5)
    ref64, _, g64 = _oracle(model, iphi, xy, rr, sigma, torch.float64, CFG, 1)
    model.to(host_device), iphi.to(host_device)
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    out = model(dev(xy), code=dev(rr), iphi=iphi)
    assert rel_l2(out.detach().cpu().numpy(), ref64) < FWD_TOL
    pmo.rel_l2_loss(out, dev(sigma)).backward()
    for k, p in model.named_parameters():
        assert rel_l2(p.grad.cpu().numpy(), g64["model." + k]) < GRAD_TOL, k


def test_explicit_points_without_iphi(host_device):
    """is_mesh=False with x_in != x_out, iphi=None, three layers (a middle layer runs); gradients reach ws."""
    model, _ = _build(3, seed=7, is_mesh=False)
    xy, _, _ = _io(N, 8)
    x_out, _, sigma = _io(50, 9)
    ref64, _, g64 = _oracle(model, None, xy, None, sigma, torch.float64, CFG, 3, x_out=x_out)
    model.to(host_device)
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    with pytest.raises(ValueError, match="x_in and x_out"):
        model(dev(xy))
    out = model(dev(xy), x_in=dev(xy), x_out=dev(x_out))
    assert out.shape == (B, 50, 1)
    assert rel_l2(out.detach().cpu().numpy(), ref64) < FWD_TOL
    pmo.rel_l2_loss(out, dev(sigma)).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad.cpu().numpy(), g64["model." + k]) < GRAD_TOL, k


def test_mesh_model_without_iphi(host_device):
    model, _ = _build(2, seed=11)
    xy, _, _ = _io(N, 12)
    ref64 = _oracle(model, None, xy, None, None, torch.float64, CFG, 2, grads=False)
    model.to(host_device)
    with torch.no_grad():
        out = model(torch.tensor(xy, device=host_device))
    assert rel_l2(out.cpu().numpy(), ref64) < FWD_TOL


@pytest.mark.gpu
def test_model_forward_at_the_shipped_big_shape(host_device="cuda:0"):
    """(Device only: the emulator needs 20 s for this shape.)  geo-fno-big: width 64, 16 modes, 64 x 64 latent grid, 972 points, 4 layers, IPhi width 64, batch 2.  xi's fp32 rounding
    times 2 pi 16 sits near 1e-5, so the band is the one of tests/test_pointcloud_model.py at this width:
    max(1e-5, 4 x the fp32 restatement's own distance from float64)."""
    cfg = dict(modes1=16, modes2=16, width=64, s1=64, s2=64)
    model, iphi = _build(4, seed=3, iphi_w=64, **cfg)
    xy, rr, sigma = _io(972, 4, b=2)
    ref64 = _oracle(model, iphi, xy, rr, sigma, torch.float64, cfg, 4, grads=False)
    noise = rel_l2(_oracle(model, iphi, xy, rr, sigma, torch.float32, cfg, 4, grads=False), ref64)
    model.to(host_device), iphi.to(host_device)
    with torch.no_grad():
        out = model(torch.tensor(xy, device=host_device), code=torch.tensor(rr, device=host_device), iphi=iphi)
    e = rel_l2(out.cpu().numpy(), ref64)
    print(f"[big] forward vs float64 {e:.2e}; the fp32 restatement's own distance {noise:.2e}")
    assert e < max(1e-5, 4 * noise)


def test_cpu_tensors_raise():
    from fourierflow_amd import _lib
    model, iphi = _build()
    with pytest.raises(_lib.FFNOLibraryError):
        model(torch.zeros(1, 10, 2), code=torch.zeros(1, 42), iphi=iphi)        # HIP only
    with pytest.raises(_lib.FFNOLibraryError):
        model(torch.zeros(1, 10, 2))


def test_shapes_outside_the_kernel_set_are_refused(host_device):
    model, _ = _build()
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    xy = _io(N, 1)[0]
    wide, _ = _build(2, width=48)
    with pytest.raises(ValueError):
        wide.to(host_device)(dev(xy))
    many, _ = _build(2, modes1=17, modes2=17, s1=40, s2=40)
    with pytest.raises(ValueError):
        many.to(host_device)(dev(xy))
    with pytest.raises(ValueError):
        model.to(host_device)(dev(np.zeros((B, N, 3), np.float32)))
