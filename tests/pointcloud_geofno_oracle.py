"""Torch restatement, in any dtype, of the geo-FNO elasticity baseline FNOPointCloud2D (reference
fourierflow/modules/zongyi_fno/point_cloud_2d.py:155-253), written from its formulas:

    V   = mix_0( fft2d(fc0(u), xi_in) )                corners [:m1] x weights1, [-m1:] x weights2
    uc  = gelu( irfft2(V, s1 x s2) + bs[0](grid) )
    uc  = gelu( irfft2(mix_i(rfft2(uc))) + ws[i-1](uc) + bs[i](grid) )      i = 1 .. L-1
    t   = ifft2d( mix_L(rfft2(uc)), xi_out )
    y   = fc2( gelu( fc1( t + bs[L](x_out) ) ) )

The non-uniform transforms, IPhi and the output head are those of tests/pointcloud_model_oracle.py.  float64 is the oracle,
float32 measures the op sequence's own rounding noise; torch autograd supplies independent gradients."""
import torch

import pointcloud_model_oracle as pmo


def _mix(ft, w1, w2, m1, m2):
    return torch.cat([torch.einsum("bixy,ioxy->boxy", ft[:, :, :m1, :m2], w1),
                      torch.einsum("bixy,ioxy->boxy", ft[:, :, -m1:, :m2], w2)], dim=-2)


def model(sd, u, code, *, modes1, modes2, width, n_layers, s1, s2, iphi_sd=None, iphi_width=None, x_in=None, x_out=None):
    """sd: reference-layout state dict of one real dtype (convs.*.weights1/2 complex); u [B, N, in] -> [B, N, out]."""
    F = torch.nn.functional
    dt = u.dtype
    x_in = u if x_in is None else x_in
    x_out = u if x_out is None else x_out
    warp = (lambda x: x) if iphi_sd is None else (lambda x: pmo.iphi(iphi_sd, x, code, iphi_width))
    xi_in = warp(x_in)
    xi_out = xi_in if x_out is x_in else warp(x_out)
    B, L = u.shape[0], n_layers
    grid = pmo.latent_grid(s1, s2, dt).to(u.device)

    def to_grid(corners):
        ft = torch.zeros(B, width, s1, s2 // 2 + 1, dtype=pmo._cdtype(dt), device=u.device)
        ft[:, :, :modes1, :modes2] = corners[:, :, :modes1]
        ft[:, :, -modes1:, :modes2] = corners[:, :, modes1:]
        return torch.fft.irfft2(ft, s=(s1, s2))

    def bs(i):
        return torch.einsum("oi,ixy->oxy", sd[f"bs.{i}.weight"].reshape(width, 2), grid) + sd[f"bs.{i}.bias"][:, None, None]

    h = F.linear(u, sd["fc0.weight"], sd["fc0.bias"]).permute(0, 2, 1)
    V = pmo.fft2d(h, xi_in, modes1, modes2)                              # corners [B, W, 2 m1, m2]
    V = torch.cat([torch.einsum("bixy,ioxy->boxy", V[:, :, :modes1], sd["convs.0.weights1"]),
                   torch.einsum("bixy,ioxy->boxy", V[:, :, modes1:], sd["convs.0.weights2"])], dim=-2)
    uc = F.gelu(to_grid(V) + bs(0))
    for i in range(1, L):
        spec = to_grid(_mix(torch.fft.rfft2(uc), sd[f"convs.{i}.weights1"], sd[f"convs.{i}.weights2"], modes1, modes2))
        lin = torch.einsum("oi,bixy->boxy", sd[f"ws.{i - 1}.weight"].reshape(width, width), uc) + sd[f"ws.{i - 1}.bias"][:, None, None]
        uc = F.gelu(spec + lin + bs(i))
    t = pmo.ifft2d(_mix(torch.fft.rfft2(uc), sd[f"convs.{L}.weights1"], sd[f"convs.{L}.weights2"], modes1, modes2), xi_out)
    head = {"bs.weight": sd[f"bs.{L}.weight"].reshape(width, 2), "bs.bias": sd[f"bs.{L}.bias"], "fc1.weight": sd["fc1.weight"],
            "fc1.bias": sd["fc1.bias"], "fc2.weight": sd["fc2.weight"], "fc2.bias": sd["fc2.bias"]}
    return pmo.point_head(head, t, x_out)
