"""The fully factorised point-cloud F-FNO's host layer: the four per-axis ops of fourierflow_amd/ops.py against torch.fft /
einsum in float64, and FNOFullyFactorizedMesh2D + IPhi against BOTH the reference's own fp32 numbers
(tests/golden/pointcloud_fullyfact_ref.npz) and the float64 restatement of tests/pointcloud_fullyfact_oracle.py -- forward
<= 1e-5, every gradient of the model and of IPhi through oracle_util.check_grads_at_rounding_level (5e-5, or 4 x the fp32
restatement's own rounding noise where a gradient is cancellation-limited): the project's bounds, as in
tests/test_pointcloud_model.py.  On the emulator and on an MI355X.

The model exposes no ReLU active sets, so before any gradient comparison the test asserts ON THE FLOAT64 ORACLE ALONE that every
feed-forward pre-activation (there are n_layers feed-forwards) is at least 1e-5 x rms(its layer) away from zero, so that no
correct fp32 evaluation can sit on another linear piece.  No unit is exempted: a flip fails the test."""
import numpy as np
import pytest
import torch

import oracle_util as ou
import pointcloud_model_oracle as pmo
from backend_util import host_device, rel_l2  # noqa: F401  (host_device is a fixture)
from test_pointcloud_fullyfact_golden import B, CFG, GOLD, N, N_LAYERS, W, build, golden_sd, oracle

FWD_TOL, GRAD_TOL = 1e-5, 5e-5


def _cplx(shape, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def _vr(z):
    return torch.view_as_real(z).detach().cpu().numpy()


# (modes1, modes2, channels, points): unequal modes both ways, the in + 1 = 3 channels of layer 0 and a width, a ragged tile and
# a tile turn-over
@pytest.mark.parametrize("m1,m2,C,n", [(3, 2, 3, 37), (2, 5, 32, 130), (12, 12, 9, 70)])
def test_point_axis_ops_against_float64(host_device, m1, m2, C, n):
    from fourierflow_amd import ops
    rng = np.random.default_rng(m1 + m2 + C)
    u = rng.standard_normal((B, C, n)).astype(np.float32)
    xi = rng.uniform(-0.45, 1.6, (B, n, 2)).astype(np.float32)
    ut, xt = (torch.tensor(a, device=host_device).requires_grad_(True) for a in (u, xi))
    u64, x64 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (u, xi))
    k2, k1 = torch.arange(m2, dtype=torch.float64), torch.arange(m1, dtype=torch.float64)
    E = torch.cat([torch.exp(2j * np.pi * x64[..., 0, None] * k2), torch.exp(2j * np.pi * x64[..., 1, None] * k1)], dim=-1)

    spec = ops.point_axis_fft(ut, xt, m1, m2)
    assert spec.dtype == torch.complex64 and spec.shape == (B, C, m2 + m1)
    ref = torch.einsum("bcn,bnt->bct", u64 + 0j, E.conj())
    assert rel_l2(_vr(spec), _vr(ref)) < FWD_TOL
    g = _cplx((B, C, m1 + m2), 5)
    du, dxi = torch.autograd.grad(spec, (ut, xt), torch.tensor(g, device=host_device))
    rdu, rdxi = torch.autograd.grad(ref, (u64, x64), torch.tensor(g.astype(np.complex128)), retain_graph=True)      # (E is used again)
    assert rel_l2(du.cpu().numpy(), rdu.numpy()) < GRAD_TOL and rel_l2(dxi.cpu().numpy(), rdxi.numpy()) < GRAD_TOL

    V = _cplx((B, C, m1 + m2), 6)
    Vt = torch.tensor(V, device=host_device).requires_grad_(True)
    V64 = torch.tensor(V.astype(np.complex128), requires_grad=True)
    out = ops.point_axis_ifft(Vt, xt, modes2=m2)
    assert out.dtype == torch.float32 and out.shape == (B, C, n)
    ref = torch.einsum("bct,bnt->bcn", V64, E).real
    assert rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < FWD_TOL
    go = rng.standard_normal((B, C, n)).astype(np.float32)
    dV, dxi = torch.autograd.grad(out, (Vt, xt), torch.tensor(go, device=host_device))
    rdV, rdxi = torch.autograd.grad(ref, (V64, x64), torch.tensor(go, dtype=torch.float64))
    assert rel_l2(_vr(dV), _vr(rdV)) < GRAD_TOL and rel_l2(dxi.cpu().numpy(), rdxi.numpy()) < GRAD_TOL
    if m1 == m2:      # modes2 = None means an even split
        assert torch.equal(ops.point_axis_ifft(Vt, xt), out)


# (S, modes1, modes2): a Nyquist mode on an even grid, an odd grid, the shipped grid
@pytest.mark.parametrize("s,m1,m2", [(8, 5, 3), (9, 4, 5), (40, 12, 12)])
def test_axis_grid_ops_against_torch_fft(host_device, s, m1, m2):
    from fourierflow_amd import ops
    V = _cplx((B, W, m1 + m2), 7 + s)
    Vt = torch.tensor(V, device=host_device).requires_grad_(True)
    V64 = torch.tensor(V.astype(np.complex128), requires_grad=True)

    def pad_irfft(z):
        full = torch.zeros(B, W, s // 2 + 1, dtype=torch.complex128)
        full[..., :z.shape[-1]] = z
        return torch.fft.irfft(full, n=s, dim=-1)
    out = ops.axis_modes_to_grid(Vt, s, modes2=m2)
    assert out.shape == (B, s, s, W)
    ref = (pad_irfft(V64[..., m2:])[:, :, :, None] + pad_irfft(V64[..., :m2])[:, :, None, :]).permute(0, 2, 3, 1)
    assert rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < FWD_TOL
    g = np.random.default_rng(8).standard_normal((B, s, s, W)).astype(np.float32)
    dV, = torch.autograd.grad(out, (Vt,), torch.tensor(g, device=host_device))
    rdV, = torch.autograd.grad(ref, (V64,), torch.tensor(g, dtype=torch.float64))
    assert rel_l2(_vr(dV), _vr(rdV)) < GRAD_TOL

    x = np.random.default_rng(9).standard_normal((B, s, s, W)).astype(np.float32)
    xt = torch.tensor(x, device=host_device).requires_grad_(True)
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    spec = ops.grid_to_axis_modes(xt, m1, m2)
    assert spec.dtype == torch.complex64 and spec.shape == (B, W, m2 + m1)
    cf = x64.permute(0, 3, 1, 2)
    ref = torch.cat([torch.fft.rfft(cf.sum(dim=2), dim=-1)[..., :m2], torch.fft.rfft(cf.sum(dim=3), dim=-1)[..., :m1]], dim=-1)
    assert rel_l2(_vr(spec), _vr(ref)) < FWD_TOL
    gs = _cplx((B, W, m1 + m2), 10)
    dx, = torch.autograd.grad(spec, (xt,), torch.tensor(gs, device=host_device))
    rdx, = torch.autograd.grad(ref, (x64,), torch.tensor(gs.astype(np.complex128)))
    assert rel_l2(dx.cpu().numpy(), rdx.numpy()) < GRAD_TOL


def test_ops_check_their_arguments(host_device):
    from fourierflow_amd import ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=host_device)      # noqa: E731
    with pytest.raises(ValueError):
        ops.point_axis_fft(z(2, 3, 10), z(2, 10, 2), 33, 2)            # modes outside the compiled set
    with pytest.raises(ValueError):
        ops.point_axis_fft(z(2, 3, 10), z(2, 9, 2), 2, 2)              # xi does not match u
    with pytest.raises(ValueError):
        ops.point_axis_fft(z(2, 3), z(2, 10, 2), 2, 2)
    with pytest.raises(TypeError):
        ops.point_axis_ifft(z(2, 3, 4), z(2, 10, 2))                   # spec must be complex64
    with pytest.raises(ValueError):
        ops.point_axis_ifft(z(2, 3, 5, dtype=torch.complex64), z(2, 10, 2))      # 5 modes: modes2 is needed
    with pytest.raises(ValueError):
        ops.axis_modes_to_grid(z(2, 32, 12, dtype=torch.complex64), 8)  # 6 modes > 8 // 2 + 1
    with pytest.raises(ValueError):
        ops.grid_to_axis_modes(z(2, 8, 9, 32), 2, 2)                   # not square
    with pytest.raises(ValueError):
        ops.grid_to_axis_modes(z(2, 8, 8, 32), 6, 2)


def test_ops_refuse_cpu_tensors():
    from fourierflow_amd import _lib, ops
    with pytest.raises(_lib.FFNOLibraryError):
        ops.point_axis_fft(torch.zeros(2, 3, 10), torch.zeros(2, 10, 2), 2, 2)      # HIP only
    with pytest.raises(_lib.FFNOLibraryError):
        ops.point_axis_ifft(torch.zeros(2, 3, 4, dtype=torch.complex64), torch.zeros(2, 10, 2))
    with pytest.raises(_lib.FFNOLibraryError):
        ops.axis_modes_to_grid(torch.zeros(2, 32, 4, dtype=torch.complex64), 8)
    with pytest.raises(_lib.FFNOLibraryError):
        ops.grid_to_axis_modes(torch.zeros(2, 8, 8, 32), 2, 2)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _io(n, seed, b=B):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.05, 0.95, (b, n, 2)).astype(np.float32), rng.standard_normal((b, 42)).astype(np.float32),
            rng.standard_normal((b, n, 1)).astype(np.float32))


def _assert_relu_margin(label, pre, n_layers):
    assert len(pre) == n_layers
    for i, p in enumerate(pre):
        margin = float(p.abs().min() / p.pow(2).mean().sqrt())
        print(f"[{label}] feed-forward {i}: min |pre| / rms = {margin:.2e}")
        assert margin >= 1e-5


def _compare(label, model, iphi, xy, rr, sigma, cfg, n_layers, host_device, x_out=None, extra_refs=()):
    """The precondition on the float64 oracle alone, then forward and every gradient of the device model against it."""
    pre = []
    ref64, loss64, g64 = oracle(model, iphi, xy, rr, sigma, torch.float64, cfg, n_layers, x_out=x_out, pre_trace=pre)
    _assert_relu_margin(label, pre, n_layers)
    model.to(host_device), iphi.to(host_device)
    dev = lambda a: torch.tensor(np.asarray(a), device=host_device)      # noqa: E731
    if x_out is None:
        out = model(dev(xy), code=dev(rr), iphi=iphi)
    else:
        out = model(dev(xy), code=dev(rr), x_in=dev(xy), x_out=dev(x_out), iphi=iphi)
    assert out.shape == ref64.shape
    got = out.detach().cpu().numpy()
    e = rel_l2(got, ref64)
    print(f"[{label}] forward vs float64 oracle {e:.2e}")
    assert e < FWD_TOL
    for name, ref in extra_refs:
        assert rel_l2(got, ref) < FWD_TOL, name
    loss = pmo.rel_l2_loss(out, dev(sigma))
    assert abs(loss.item() - loss64) < FWD_TOL * abs(loss64)
    loss.backward()
    grads = {}
    for prefix, mod in (("model.", model), ("iphi.", iphi)):
        for k, p in mod.named_parameters():
            grads[prefix + k] = None if p.grad is None else p.grad.detach().cpu().numpy()
    skip = ("model.ws.", f"model.convs.{n_layers}.backcast_ff.", "iphi.fc_no_code.")
    unused = [k for k in grads if k.startswith(skip)]
    assert len(unused) == 2 * (n_layers - 1) + 6 + 2
    for k in unused:      # registered, never read: no gradient here and none in the oracle
        assert grads[k] is None and g64[k] is None, k
    used = {k: v for k, v in grads.items() if k not in unused}
    assert all(v is not None for v in used.values()), [k for k, v in used.items() if v is None]
    model_cpu, iphi_cpu = model.cpu(), iphi.cpu()
    cache = {torch.float64: g64}

    def run(dtype):
        if dtype not in cache:
            cache[dtype] = oracle(model_cpu, iphi_cpu, xy, rr, sigma, dtype, cfg, n_layers, x_out=x_out)[2]
        return {k: cache[dtype][k] for k in used}
    ou.check_grads_at_rounding_level(label, used, run)
    return grads


def test_model_against_the_reference_and_the_float64_restatement(host_device):
    model, iphi = build()
    model.load_state_dict(golden_sd("model")), iphi.load_state_dict(golden_sd("iphi"))
    grads = _compare("golden", model, iphi, GOLD["xy"], GOLD["rr"], GOLD["sigma"], CFG, N_LAYERS, host_device,
                     extra_refs=[("the reference's fp32 output", GOLD["out"])])
    n = 0
    for who in ("model", "iphi"):      # and every gradient against the reference's own fp32 one
        for k in GOLD.files:
            if k.startswith(f"{who}.g."):
                name = k[len(who) + 3:]
                e = rel_l2(grads[f"{who}.{name}"], GOLD[k])
                assert e < GRAD_TOL, (k, e)
                n += 1
    assert n == 40


# label -> (n_layers, modes1, modes2, S, explicit x_out, seed).  Seeds picked by the precondition above alone (float64 oracle; the
# smallest seed of 0..11 whose margin holds), before any kernel ran.
CASES = {
    "one-layer": (1, 3, 2, 8, False, 0),          # no middle layer
    "equal-modes": (3, 3, 3, 8, False, 0),        # m1 = m2: no weight padding in the middle layers
    "nyquist": (2, 5, 5, 8, False, 1),            # S = 8 with 5 modes
    "odd-grid": (2, 5, 4, 9, False, 0),           # S = 9
    "explicit-points": (2, 3, 2, 8, True, 0),     # is_mesh=False with x_in != x_out: iphi runs twice
}


def case_inputs(label):
    n_layers, m1, m2, s, explicit, seed = CASES[label]
    cfg = dict(modes1=m1, modes2=m2, width=W, s=s)
    kw = dict(is_mesh=False) if explicit else {}
    model, iphi = build(n_layers, seed, **cfg, **kw)
    xy, rr, sigma = _io(N, 10 + seed)
    x_out = None
    if explicit:
        x_out, _, sigma = _io(50, 20 + seed)
    return model, iphi, xy, rr, sigma, cfg, n_layers, x_out


@pytest.mark.parametrize("label", list(CASES))
def test_model_forward_and_gradients(host_device, label):
    model, iphi, xy, rr, sigma, cfg, n_layers, x_out = case_inputs(label)
    assert len(model.ws) == n_layers - 1 and len(model.convs) == n_layers + 1 and len(model.bs) == 2
    _compare(label, model, iphi, xy, rr, sigma, cfg, n_layers, host_device, x_out=x_out)


def test_iphi_runs_once_on_shared_points(host_device):
    model, iphi = build()
    model.to(host_device), iphi.to(host_device)
    calls = []
    handle = iphi.register_forward_hook(lambda *a: calls.append(1))
    xy, rr, _ = _io(N, 3)
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    with torch.no_grad():
        model(dev(xy), code=dev(rr), iphi=iphi)
        assert len(calls) == 1
        x = dev(xy)
        model(x, code=dev(rr), x_in=x, x_out=x, iphi=iphi)
        assert len(calls) == 2
        model(x, code=dev(rr), x_in=x, x_out=dev(xy), iphi=iphi)      # equal values, another tensor: two evaluations
        assert len(calls) == 4
    handle.remove()


def test_refusals(host_device):
    from fourierflow_amd.modules import FNOFullyFactorizedMesh2D
    with pytest.raises(ValueError, match="reference fails"):
        FNOFullyFactorizedMesh2D(3, 2, W, 2, 1, s1=8, s2=10)
    with pytest.raises(ValueError, match="s1 // 2 \\+ 1"):
        FNOFullyFactorizedMesh2D(6, 2, W, 2, 1, s1=8, s2=8)
    with pytest.raises(ValueError, match="s1 // 2 \\+ 1"):
        FNOFullyFactorizedMesh2D(2, 6, W, 2, 1, s1=8, s2=8)
    dev = lambda a: torch.tensor(a, device=host_device)      # noqa: E731
    xy, rr, _ = _io(N, 1)
    model, iphi = build()
    model.to(host_device), iphi.to(host_device)
    with pytest.raises(ValueError, match="iphi"):
        model(dev(xy), code=dev(rr))
    with pytest.raises(ValueError):
        model(dev(np.zeros((B, N, 3), np.float32)), code=dev(rr), iphi=iphi)
    loose, _ = build(is_mesh=False)
    loose.to(host_device)
    with pytest.raises(ValueError, match="x_in and x_out"):
        loose(dev(xy), code=dev(rr), iphi=iphi)
    with pytest.raises(ValueError, match="x_in and x_out"):
        loose(dev(xy), code=dev(rr), x_in=dev(xy), iphi=iphi)
    wide, _ = build(width=48)
    with pytest.raises(ValueError, match="width 48"):
        wide.to(host_device)(dev(xy), code=dev(rr), iphi=iphi)
    many, _ = build(modes1=33, modes2=33, s=80)
    with pytest.raises(ValueError, match="modes \\(33, 33\\)"):
        many.to(host_device)(dev(xy), code=dev(rr), iphi=iphi)
    with pytest.raises(NotImplementedError, match="fc_no_code"):      # IPhi(code=None) stays refused
        model(dev(xy), iphi=iphi)


def test_cpu_tensors_raise():
    from fourierflow_amd import _lib
    model, iphi = build()
    with pytest.raises(_lib.FFNOLibraryError):
        model(torch.zeros(1, 10, 2), code=torch.zeros(1, 42), iphi=iphi)        # HIP only


@pytest.mark.gpu
def test_model_forward_at_the_shipped_shape(host_device="cuda:0"):
    """(Device only.)  Batch 20 x 972 points, width 32, 12 modes, 40 x 40 latent grid, 4 layers, IPhi width 32, against the fp32
    restatement.  Two correct fp32 evaluations of this op sequence differ by its own rounding noise, measured as the fp32
    restatement's distance from the float64 one; the band against float64 is the one tests/test_pointcloud_model.py uses at its
    large shape, max(1e-5, 4 x noise), and against the fp32 restatement that plus the noise itself (triangle inequality)."""
    cfg = dict(modes1=12, modes2=12, width=32, s=40)
    model, iphi = build(4, seed=3, iphi_w=32, **cfg)
    xy, rr, sigma = _io(972, 4, b=20)
    ref64 = oracle(model, iphi, xy, rr, sigma, torch.float64, cfg, 4, grads=False)
    ref32 = oracle(model, iphi, xy, rr, sigma, torch.float32, cfg, 4, grads=False)
    noise = rel_l2(ref32, ref64)
    model.to(host_device), iphi.to(host_device)
    with torch.no_grad():
        out = model(torch.tensor(xy, device=host_device), code=torch.tensor(rr, device=host_device), iphi=iphi)
    assert out.shape == (20, 972, 1)
    e32, e64 = rel_l2(out.cpu().numpy(), ref32), rel_l2(out.cpu().numpy(), ref64)
    print(f"[shipped shape] forward vs the fp32 restatement {e32:.2e}, vs float64 {e64:.2e}; the fp32 restatement's own distance {noise:.2e}")
    assert e64 < max(1e-5, 4 * noise)
    assert e32 < max(1e-5, 4 * noise) + noise
