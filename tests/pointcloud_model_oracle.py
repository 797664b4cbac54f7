"""Torch restatement, in any dtype, of the two per-point networks of the elasticity F-FNO: IPhi (reference
fourierflow/modules/iphi.py:27-58, the `code` branch) and the output head of FNOFactorizedPointCloud2D
(modules/factorized_fno/point_cloud_2d.py:263-270).  Written from the formulas so torch autograd supplies independent
gradients; float64 is the oracle, float32 measures the reference op sequence's own rounding noise."""
import numpy as np
import torch

CENTER = float(np.float32(1e-4))           # torch.tensor([0.0001, 0.0001]) of the reference is fp32
PI32 = float(np.float32(np.pi))            # np.pi * (fp32 tensor) rounds pi to fp32; the powers of two scale it exactly
CODE_DIM = 42

IPHI_NAMES = ("fc0.weight", "fc0.bias", "fc_code.weight", "fc_code.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias",
              "fc3.weight", "fc3.bias", "fc4.weight", "fc4.bias")
HEAD_NAMES = ("bs.weight", "bs.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def iphi_shapes(width):
    H = 4 * width
    return {"fc0.weight": (width, 4), "fc0.bias": (width,), "fc_code.weight": (width, CODE_DIM), "fc_code.bias": (width,),
            "fc1.weight": (H, H), "fc1.bias": (H,), "fc2.weight": (H, H), "fc2.bias": (H,), "fc3.weight": (H, H),
            "fc3.bias": (H,), "fc4.weight": (2, H), "fc4.bias": (2,)}


def head_shapes(W, out):
    return {"bs.weight": (W, 2), "bs.bias": (W,), "fc1.weight": (128, W), "fc1.bias": (128,), "fc2.weight": (out, 128),
            "fc2.bias": (out,)}


def linear_init(shapes, seed):
    """nn.Linear's default scale: weights and biases uniform in +-1/sqrt(fan_in); fp32 values."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in shapes.items():
        if name.endswith(".weight"):
            bound = 1.0 / np.sqrt(shape[1])
        sd[name] = rng.uniform(-bound, bound, shape).astype(np.float32)
    return sd


def iphi_features(x):
    """x [..., 2] -> [..., 4] = (x0, x1, angle, radius)."""
    dx, dy = x[..., 0] - CENTER, x[..., 1] - CENTER
    return torch.stack([x[..., 0], x[..., 1], torch.atan2(dy, dx), torch.sqrt(dx * dx + dy * dy)], dim=-1)


def iphi(sd, x, code, width, feat=None, fp32_products=False):
    """sd: {name: tensor} of one dtype; x [B, N, 2], code [B, 42] -> xi [B, N, 2].
    feat: use these four features instead of computing them (the kernel's own, for the staged comparison);
    fp32_products: B_k * feature rounded once to fp32 -- what an fp32 evaluation feeds sin / cos."""
    dt = x.dtype
    B, N = x.shape[:2]
    xd = iphi_features(x) if feat is None else feat.to(dt)
    nf = width // 4
    bk32 = torch.tensor([np.float32(PI32) * np.float32(2.0 ** k) for k in range(nf)], dtype=torch.float32, device=x.device)
    if fp32_products:
        arg = (xd.detach().to(torch.float32)[..., None] * bk32).to(dt)
    else:
        arg = xd[..., None] * bk32.to(dt)
    s, c = torch.sin(arg).reshape(B, N, width), torch.cos(arg).reshape(B, N, width)
    h = torch.nn.functional.linear(xd, sd["fc0.weight"], sd["fc0.bias"])
    cd = torch.nn.functional.linear(code, sd["fc_code.weight"], sd["fc_code.bias"])[:, None, :].expand(B, N, width)
    h = torch.cat([cd, h, s, c], dim=-1)
    for l in (1, 2, 3):
        h = torch.tanh(torch.nn.functional.linear(h, sd[f"fc{l}.weight"], sd[f"fc{l}.bias"]))
    h = torch.nn.functional.linear(h, sd["fc4.weight"], sd["fc4.bias"])
    return x + x * h


def point_head(sd, t, x):
    """t [B, W, N] channel-major, x [B, N, 2] -> [B, N, out]; exact (erf) GELU."""
    s = t.permute(0, 2, 1) + torch.nn.functional.linear(x, sd["bs.weight"], sd["bs.bias"])
    h = torch.nn.functional.gelu(torch.nn.functional.linear(s, sd["fc1.weight"], sd["fc1.bias"]))
    return torch.nn.functional.linear(h, sd["fc2.weight"], sd["fc2.bias"])


def to_torch(sd_np, dtype, requires_grad=False):
    return {k: torch.tensor(v, dtype=dtype, requires_grad=requires_grad) for k, v in sd_np.items()}


# ---- the whole model (reference point_cloud_2d.py:223-270), literal op sequence, any dtype --------------------------------
def _cdtype(dt):
    return torch.complex128 if dt == torch.float64 else torch.complex64


def _basis(xi, modes1, modes2, sign):
    """exp(sign 2 pi i (k1 xi_1 + k2 xi_2)) on the reference's full 2 modes1 x (2 modes2 - 1) wavenumber set, in xi's dtype."""
    dt = xi.dtype
    k1 = torch.cat((torch.arange(0, modes1), torch.arange(-modes1, 0))).to(dt).to(xi.device)
    k2 = torch.cat((torch.arange(0, modes2), torch.arange(-(modes2 - 1), 0))).to(dt).to(xi.device)
    K = xi[..., 0, None, None] * k1[:, None] + xi[..., 1, None, None] * k2[None, :]
    return torch.exp(sign * 1j * 2 * np.pi * K)


def fft2d(h, xi, modes1, modes2):
    if h.dtype == torch.float64:
        import pointcloud_oracle as po
        return po.fft2d(h, xi, modes1, modes2)
    Y = torch.einsum("bcn,bnxy->bcxy", h + 0j, _basis(xi, modes1, modes2, -1))
    return torch.cat([Y[:, :, :modes1, :modes2], Y[:, :, -modes1:, :modes2]], dim=-2)


def ifft2d(spec, xi):
    if spec.dtype == torch.complex128:
        import pointcloud_oracle as po
        return po.ifft2d(spec, xi)
    modes1, modes2 = spec.shape[2] // 2, spec.shape[3]
    full = torch.cat([spec, spec[..., 1:].flip(-1, -2).conj()], dim=-1)
    return torch.einsum("bcxy,bnxy->bcn", full, _basis(xi, modes1, modes2, 1)).real


def latent_grid(s1, s2, dtype):
    """[2, s1, s2]: fp32 linspace(0, 1, s) with the end point (get_grid, :272-280), cast to dtype."""
    gx = torch.tensor(np.linspace(0, 1, s1), dtype=torch.float).reshape(s1, 1).repeat(1, s2)
    gy = torch.tensor(np.linspace(0, 1, s2), dtype=torch.float).reshape(1, s2).repeat(s1, 1)
    return torch.stack([gx, gy]).to(dtype)


def model(sd, u, code, *, modes1, modes2, width, n_layers, s1, s2, iphi_sd=None, iphi_width=None, x_in=None, x_out=None,
          pre_trace=None):
    """sd: reference-layout state dict of one real dtype (convs.{n_layers}.weights1/2 complex).  pre_trace: a list that
    receives every feed-forward pre-activation [pixels, hidden] (the ReLU inputs)."""
    from oracle import ffno_oracle as orc
    F = torch.nn.functional
    dt = u.dtype
    x_in = u if x_in is None else x_in
    x_out = u if x_out is None else x_out
    warp = (lambda x: x) if iphi_sd is None else (lambda x: iphi(iphi_sd, x, code, iphi_width))
    xi_in = warp(x_in)
    xi_out = xi_in if x_out is x_in else warp(x_out)
    h = F.linear(u, sd["fc0.weight"], sd["fc0.bias"]).permute(0, 2, 1)
    V = fft2d(h, xi_in, modes1, modes2)
    B = u.shape[0]

    def to_grid(corners):
        ft = torch.zeros(B, width, s1, s2 // 2 + 1, dtype=_cdtype(dt), device=u.device)
        ft[:, :, :modes1, :modes2] = corners[:, :, :modes1]
        ft[:, :, -modes1:, :modes2] = corners[:, :, modes1:]
        return torch.fft.irfft2(ft, s=(s1, s2))

    G = torch.einsum("oi,ixy->oxy", sd["bs.0.weight"].reshape(width, 2), latent_grid(s1, s2, dt).to(u.device)) + sd["bs.0.bias"][:, None, None]
    uc = to_grid(V) + G
    for i in range(1, n_layers):
        xs = orc.forward_fourier(uc.permute(0, 2, 3, 1), sd[f"convs.{i}.fourier_weight.0"], sd[f"convs.{i}.fourier_weight.1"], modes1)
        prefix = f"convs.{i}.backcast_ff."
        if pre_trace is not None:
            pre_trace.append(orc.linear_from_sd(sd, prefix + "layers.0.0.", xs).detach().reshape(-1, 2 * width))
        uc = uc + orc.feedforward(sd, prefix, xs).permute(0, 3, 1, 2) + G
    L = n_layers
    ft = torch.fft.rfft2(uc)
    f1 = torch.einsum("bixy,ioxy->boxy", ft[:, :, :modes1, :modes2], sd[f"convs.{L}.weights1"])
    f2 = torch.einsum("bixy,ioxy->boxy", ft[:, :, -modes1:, :modes2], sd[f"convs.{L}.weights2"])
    t = ifft2d(torch.cat([f1, f2], dim=-2), xi_out)
    head = {"bs.weight": sd["bs.1.weight"].reshape(width, 2), "bs.bias": sd["bs.1.bias"], "fc1.weight": sd["fc1.weight"],
            "fc1.bias": sd["fc1.bias"], "fc2.weight": sd["fc2.weight"], "fc2.bias": sd["fc2.bias"]}
    return point_head(head, t, x_out)


def model_state_dict(module_sd, dtype, requires_grad=True):
    """A module's state_dict -> ({key: tensor}, {unique name: leaf}) in dtype (complex weights in the matching complex dtype);
    keys that share storage (shared Fourier weights) alias one leaf."""
    uniq, sd, first = {}, {}, {}
    for k, v in module_sd.items():
        ck = first.setdefault(v.data_ptr(), k)        # shared tensors: the first key is the name named_parameters() reports
        if ck not in uniq:
            v = v.detach().cpu()
            v = v.to(_cdtype(dtype) if v.is_complex() else dtype).clone()
            uniq[ck] = v.requires_grad_(requires_grad)
        sd[k] = uniq[ck]
    return sd, uniq


def rel_l2_loss(pred, target):
    """mean_b ||pred_b - target_b||_2 / ||target_b||_2 (LpLoss(size_average=True) of routines/point_cloud.py)."""
    B = pred.shape[0]
    d = (pred.reshape(B, -1) - target.reshape(B, -1)).norm(dim=1)
    return (d / target.reshape(B, -1).norm(dim=1)).mean()
