"""The elasticity F-FNO's host layer: the grid <-> corner-mode ops of fourierflow_amd/ops.py against torch.fft in float64,
and FNOFactorizedPointCloud2D + IPhi against the float64 restatement of tests/pointcloud_model_oracle.py -- forward <= 1e-5,
every gradient of the model and of IPhi through oracle_util.check_grads_at_rounding_level (5e-5, or 4 x the fp32
restatement's own rounding noise where a gradient is cancellation-limited).  On the emulator and on an MI355X.

The model exposes no ReLU active sets, so before any gradient comparison the test asserts ON THE FLOAT64 ORACLE ALONE that
every feed-forward pre-activation is at least 1e-5 x rms(its layer) away from zero -- about 30 times the expected fp32
error -- so that no correct fp32 evaluation can sit on another linear piece.  No unit is exempted: a flip fails the test."""
import numpy as np
import pytest
import torch

import oracle_util as ou
import pointcloud_model_oracle as pmo
import test_kernels_iphi as tki
import test_kernels_pchead as tkp
from backend_util import Backend, host_device, rel_l2  # noqa: F401  (host_device is a fixture)

B, W, M1, M2, S1, S2, N = 2, 32, 4, 3, 10, 12, 37      # unequal modes and grid axes catch swaps; 37 points: a ragged tile
IPHI_W = 16


def _cplx(shape, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def test_corners_to_grid_is_irfft2(host_device):
    from fourierflow_amd import ops
    V = _cplx((B, W, 2 * M1, M2), 1)
    Vt = torch.tensor(V, device=host_device).requires_grad_(True)
    out = ops.corners_to_grid(Vt, S1, S2)
    assert out.shape == (B, S1, S2, W)
    V64 = torch.tensor(V.astype(np.complex128), requires_grad=True)
    ft = torch.zeros(B, W, S1, S2 // 2 + 1, dtype=torch.complex128)
    ft[:, :, :M1, :M2] = V64[:, :, :M1]
    ft[:, :, -M1:, :M2] = V64[:, :, M1:]
    ref = torch.fft.irfft2(ft, s=(S1, S2)).permute(0, 2, 3, 1)
    assert rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    g = np.random.default_rng(2).standard_normal((B, S1, S2, W)).astype(np.float32)
    dV, = torch.autograd.grad(out, (Vt,), torch.tensor(g, device=host_device))
    rdV, = torch.autograd.grad(ref, (V64,), torch.tensor(g, dtype=torch.float64))
    assert rel_l2(torch.view_as_real(dV).cpu().numpy(), torch.view_as_real(rdV).numpy()) < 5e-5


def test_grid_to_mixed_corners_is_rfft2_and_mix(host_device):
    from fourierflow_amd import ops
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, S1, S2, W)).astype(np.float32)
    w1, w2 = _cplx((W, W, M1, M2), 4, 1 / W), _cplx((W, W, M1, M2), 5, 1 / W)
    xt = torch.tensor(x, device=host_device).requires_grad_(True)
    w1t = torch.view_as_real(torch.tensor(w1, device=host_device)).clone().requires_grad_(True)
    w2t = torch.view_as_real(torch.tensor(w2, device=host_device)).clone().requires_grad_(True)
    out = ops.grid_to_mixed_corners(xt, w1t, w2t)
    assert out.shape == (B, W, 2 * M1, M2) and out.dtype == torch.complex64
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    w164 = torch.tensor(w1.astype(np.complex128), requires_grad=True)
    w264 = torch.tensor(w2.astype(np.complex128), requires_grad=True)
    ft = torch.fft.rfft2(x64.permute(0, 3, 1, 2))
    ref = torch.cat([torch.einsum("bixy,ioxy->boxy", ft[:, :, :M1, :M2], w164),
                     torch.einsum("bixy,ioxy->boxy", ft[:, :, -M1:, :M2], w264)], dim=-2)
    assert rel_l2(torch.view_as_real(out).detach().cpu().numpy(), torch.view_as_real(ref).detach().numpy()) < 1e-5
    g = _cplx((B, W, 2 * M1, M2), 6)
    dx, d1, d2 = torch.autograd.grad(out, (xt, w1t, w2t), torch.tensor(g, device=host_device))
    rdx, r1, r2 = torch.autograd.grad(ref, (x64, w164, w264), torch.tensor(g.astype(np.complex128)))
    assert rel_l2(dx.cpu().numpy(), rdx.numpy()) < 5e-5
    assert rel_l2(d1.cpu().numpy(), torch.view_as_real(r1).numpy()) < 5e-5
    assert rel_l2(d2.cpu().numpy(), torch.view_as_real(r2).numpy()) < 5e-5


def test_grid_ops_refuse_modes_that_do_not_fit(host_device):
    from fourierflow_amd import ops
    with pytest.raises(ValueError):      # 2 modes1 > s1
        ops.corners_to_grid(torch.zeros(B, W, 12, M2, dtype=torch.complex64, device=host_device), S1, S2)
    with pytest.raises(ValueError):      # modes2 > s2 // 2
        ops.corners_to_grid(torch.zeros(B, W, 2 * M1, 7, dtype=torch.complex64, device=host_device), S1, S2)
    with pytest.raises(ValueError):
        ops.grid_to_mixed_corners(torch.zeros(B, S1, S2, W, device=host_device), torch.zeros(W, W, 6, M2, 2, device=host_device),
                                  torch.zeros(W, W, 6, M2, 2, device=host_device))


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _build(n_layers, share, seed, width=W, m1=M1, m2=M2, s1=S1, s2=S2, iphi_w=IPHI_W):
    from fourierflow_amd.modules import FNOFactorizedPointCloud2D, IPhi
    torch.manual_seed(seed)
    model = FNOFactorizedPointCloud2D(m1, m2, width, 2, 1, n_layers=n_layers, s1=s1, s2=s2, share_weight=share)
    iphi = IPhi(iphi_w)
    return model, iphi


def _io(n, seed, b=B):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.05, 0.95, (b, n, 2)).astype(np.float32)
    rr = rng.standard_normal((b, 42)).astype(np.float32)
    sigma = rng.standard_normal((b, n, 1)).astype(np.float32)
    return xy, rr, sigma


def _oracle_run(model, iphi, xy, rr, sigma, dtype, cfg, pre_trace=None, grads=True):
    sd, uniq = pmo.model_state_dict(model.state_dict(), dtype)
    isd, iuniq = pmo.model_state_dict(iphi.state_dict(), dtype)
    out = pmo.model(sd, torch.tensor(xy, dtype=dtype), torch.tensor(rr, dtype=dtype), iphi_sd=isd, iphi_width=iphi.width,
                    pre_trace=pre_trace, **cfg)
    if not grads:
        return out.detach().numpy()
    pmo.rel_l2_loss(out, torch.tensor(sigma, dtype=dtype)).backward()

    def g(t):
        if t.grad is None:
            return None
        return (torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad).numpy()
    res = {"model." + k: g(v) for k, v in uniq.items()}
    res.update({"iphi." + k: g(v) for k, v in iuniq.items()})
    return out.detach().numpy(), res


# seeds picked by the precondition above alone (float64 oracle; margins of seeds 3..11: 2.8e-6 .. 4.2e-4), before any kernel ran
SEEDS = {(3, False): 4, (3, True): 9, (1, False): 2}


@pytest.mark.parametrize("n_layers,share", list(SEEDS))
def test_model_forward_and_gradients(host_device, n_layers, share):
    cfg = dict(modes1=M1, modes2=M2, width=W, n_layers=n_layers, s1=S1, s2=S2)
    seed = SEEDS[(n_layers, share)]
    model, iphi = _build(n_layers, share, seed)
    xy, rr, sigma = _io(N, 10 + seed)

    # precondition, on the float64 oracle alone: no ReLU input near zero
    pre = []
    ref64, g64 = _oracle_run(model, iphi, xy, rr, sigma, torch.float64, cfg, pre_trace=pre)
    assert len(pre) == n_layers - 1
    for i, p in enumerate(pre):
        margin = float(p.abs().min() / p.pow(2).mean().sqrt())
        print(f"[n_layers={n_layers} share={share}] feed-forward {i + 1}: min |pre| / rms = {margin:.2e}")
        assert margin >= 1e-5

    model.to(host_device), iphi.to(host_device)
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    out = model(dev(xy), code=dev(rr), iphi=iphi)
    assert out.shape == (B, N, 1)
    e = rel_l2(out.detach().cpu().numpy(), ref64)
    print(f"[n_layers={n_layers} share={share}] forward vs float64 oracle {e:.2e}")
    assert e < 1e-5

    pmo_loss = pmo.rel_l2_loss(out, dev(sigma))
    pmo_loss.backward()
    grads = {}
    for prefix, mod in (("model.", model), ("iphi.", iphi)):
        for k, p in mod.named_parameters():
            grads[prefix + k] = None if p.grad is None else p.grad.detach().cpu().numpy()
    unused = [k for k in grads if k.startswith("model.ws.") or k.startswith("iphi.fc_no_code.")]
    assert len(unused) == 2 * (n_layers - 1) + 2
    for k in unused:
        assert grads[k] is None and g64[k] is None, k
    used = {k: v for k, v in grads.items() if k not in unused}
    assert all(v is not None for v in used.values()), [k for k, v in used.items() if v is None]
    cache = {torch.float64: g64}

    def run(dtype):
        if dtype not in cache:
            cache[dtype] = _oracle_run(model_cpu, iphi_cpu, xy, rr, sigma, dtype, cfg)[1]
        return {k: cache[dtype][k] for k in used}
    model_cpu, iphi_cpu = model.cpu(), iphi.cpu()
    ou.check_grads_at_rounding_level(f"pointcloud n_layers={n_layers} share={share}", used, run)


def test_explicit_points_and_no_iphi(host_device):
    cfg = dict(modes1=M1, modes2=M2, width=W, n_layers=2, s1=S1, s2=S2)
    model, _ = _build(2, False, 7)
    xy, _, _ = _io(N, 8)
    x_out = _io(50, 9)[0]
    sd, _ = pmo.model_state_dict(model.state_dict(), torch.float64, requires_grad=False)
    ref = pmo.model(sd, torch.tensor(xy, dtype=torch.float64), None, x_in=torch.tensor(xy, dtype=torch.float64),
                    x_out=torch.tensor(x_out, dtype=torch.float64), **cfg).numpy()
    model.to(host_device)
    with torch.no_grad():
        out = model(torch.tensor(xy, device=host_device), x_in=torch.tensor(xy, device=host_device),
                    x_out=torch.tensor(x_out, device=host_device))
    assert out.shape == (B, 50, 1)
    assert rel_l2(out.cpu().numpy(), ref) < 1e-5


def test_loud_failures():
    from fourierflow_amd import _lib
    from fourierflow_amd.modules import IPhi
    model, iphi = _build(2, False, 0)
    with pytest.raises(_lib.FFNOLibraryError):
        model(torch.zeros(1, 10, 2), code=torch.zeros(1, 42), iphi=iphi)        # CPU tensors: HIP only
    with pytest.raises(NotImplementedError, match="fc_no_code"):
        iphi(torch.zeros(1, 10, 2))
    with pytest.raises(ValueError):
        IPhi(30)


def test_iphi_refuses_a_coordinate_gradient(host_device):
    _, iphi = _build(1, False, 0)
    iphi.to(host_device)
    x = torch.rand(1, 10, 2, device=host_device).requires_grad_(True)
    xi = iphi(x, torch.zeros(1, 42, device=host_device))
    with pytest.raises(RuntimeError, match="input coordinates"):
        xi.sum().backward()


def test_autograd_wrappers_match_the_c_abi_over_slices_and_passes(host_device):
    """ops.iphi_forward at two gradient slices (width 16, 2 x 530 points) and ops.point_head at 132 tiles (W = 32, 3 x 2757
    points) under torch.autograd give the bits of the direct C ABI calls of test_kernels_iphi.py / test_kernels_pchead.py on the
    same inputs: _IPhiFn.backward and _PointHeadFn.backward size their workspaces for the slice and split counts the kernels
    use, and hand over the same buffers in the same order."""
    from fourierflow_amd import ops
    be = Backend("emu" if host_device == "cpu" else "gpu")
    dev = lambda a, grad=False: torch.tensor(a, device=host_device).requires_grad_(grad)   # noqa: E731

    width, b, n = tki.MULTI_SLICE[0]
    sd, x, code, dxi = tki._inputs(width, b, n, 200 + width)
    hp, par, hx, hc, xi, feat, acts = tki._forward(be, sd, x, code, width, True)
    grads, dcode, _ = tki.iphi_backward(be, par, hx, hc, feat, acts, sd, dxi, width)
    params = [dev(sd[k], True) for k in pmo.IPHI_NAMES]
    ct = dev(code, True)
    out = ops.iphi_forward(dev(x), ct, width, params)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), be.get(xi))
    got = torch.autograd.grad(out, [ct] + params, dev(dxi))
    np.testing.assert_array_equal(got[0].cpu().numpy(), dcode)
    for k, g in zip(pmo.IPHI_NAMES, got[1:]):
        np.testing.assert_array_equal(g.cpu().numpy(), grads[k], err_msg=k)

    w, b, n, o = tkp.MULTI_PASS[0]
    sd, t, x, dy = tkp._inputs(w, b, n, o, 300 + w + n)
    par, ht, hx, y, pre = tkp.pchead_forward(be, sd, t, x, o)
    dt, grads, _ = tkp.pchead_backward(be, par, ht, hx, pre, sd, dy)
    bs, fc1, fc2 = torch.nn.Conv1d(2, w, 1), torch.nn.Linear(w, 128), torch.nn.Linear(128, o)
    with torch.no_grad():
        bs.weight.copy_(torch.tensor(sd["bs.weight"]).reshape(w, 2, 1)), bs.bias.copy_(torch.tensor(sd["bs.bias"]))
        fc1.weight.copy_(torch.tensor(sd["fc1.weight"])), fc1.bias.copy_(torch.tensor(sd["fc1.bias"]))
        fc2.weight.copy_(torch.tensor(sd["fc2.weight"])), fc2.bias.copy_(torch.tensor(sd["fc2.bias"]))
    bs.to(host_device), fc1.to(host_device), fc2.to(host_device)
    tt = dev(t, True)
    out = ops.point_head(tt, dev(x), bs, fc1, fc2)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), be.get(y))
    mods = [bs.weight, bs.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    got = torch.autograd.grad(out, [tt] + mods, dev(dy))
    np.testing.assert_array_equal(got[0].cpu().numpy(), dt)
    for k, g in zip(pmo.HEAD_NAMES, got[1:]):
        np.testing.assert_array_equal(g.cpu().numpy().reshape(grads[k].shape), grads[k], err_msg=k)


@pytest.mark.gpu
def test_model_forward_at_the_shipped_width():
    """Width 64, 16 modes, 64 x 64 latent grid, IPhi width 32.  xi's fp32 rounding times 2 pi 16 sits near 1e-5, so the band
    is max(1e-5, 4 x the fp32 restatement's own distance from float64)."""
    cfg = dict(modes1=16, modes2=16, width=64, n_layers=2, s1=64, s2=64)
    model, iphi = _build(2, False, 3, width=64, m1=16, m2=16, s1=64, s2=64, iphi_w=32)
    xy, rr, sigma = _io(130, 4)
    ref64 = _oracle_run(model, iphi, xy, rr, sigma, torch.float64, cfg, grads=False)
    ref32 = _oracle_run(model, iphi, xy, rr, sigma, torch.float32, cfg, grads=False)
    noise = rel_l2(ref32, ref64)
    model.cuda(), iphi.cuda()
    with torch.no_grad():
        out = model(torch.tensor(xy).cuda(), code=torch.tensor(rr).cuda(), iphi=iphi)
    e = rel_l2(out.cpu().numpy(), ref64)
    print(f"[width 64] forward vs float64 oracle {e:.2e}; the fp32 restatement's own distance {noise:.2e}")
    assert e < max(1e-5, 4 * noise)
