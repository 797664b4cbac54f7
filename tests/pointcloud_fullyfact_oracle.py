"""Torch restatement, in any dtype, of the fully factorised point-cloud F-FNO FNOFullyFactorizedMesh2D (reference
fourierflow/modules/factorized_fno/mesh_plus_2d.py:14-280), written from its formulas in their separable form (S = s1 = s2;
coordinate 0 of xi pairs with the last grid axis y, modes2 and fourier_weight[0]; coordinate 1 with the first axis x, modes1 and
fourier_weight[1]):

    Ay[b,c,j] = sum_n fc0(u)[b,c,n] exp(-2 pi i j xi[b,n,0]),  Ax[b,c,k] likewise with xi[b,n,1]
    s[b,:,x,y] = irfft(pad(mix_x(Ax)), n=S)[x] + irfft(pad(mix_y(Ay)), n=S)[y]          mix: "bik,iok->bok"
    uc = backcast_0(s) + G,  G = bs[0](grid)
    uc = uc + backcast_i( irfft_y(pad(mix_y(rfft_y(uc)[:m2]))) + irfft_x(pad(mix_x(rfft_x(uc)[:m1]))) ) + G      i = 1 .. L-1
    t[b,o,n] = Re sum_j mix_y(rfft_y(sum_x uc))[b,o,j] exp(2 pi i j xi[b,n,0]) + the same in x with xi[b,n,1]
    y = fc2(gelu(fc1(t + bs[1](x_out))))

The reference repeats its one-dimensional bases along the other grid axis and sums over it again; the sums are taken here once.
IPhi and the output head are those of tests/pointcloud_model_oracle.py, the feed-forward the one of oracle/ffno_oracle.py.
float64 is the oracle, float32 measures the op sequence's own rounding noise; torch autograd supplies independent gradients."""
import numpy as np
import torch

import pointcloud_model_oracle as pmo


def _modes_of(x, coord, m, sign):
    """exp(sign 2 pi i k x[..., coord]) for k < m: [B, N, m] in x's precision"""
    k = torch.arange(m, dtype=x.dtype, device=x.device)
    return torch.exp(sign * 2j * np.pi * (x[..., coord, None] * k))


def _irfft_padded(z, S, dim):
    """irfft(n = S) along dim of the spectrum z zero-padded there to S // 2 + 1 bins"""
    z = z.movedim(dim, -1)
    full = z.new_zeros(z.shape[:-1] + (S // 2 + 1,))
    full[..., :z.shape[-1]] = z
    return torch.fft.irfft(full, n=S, dim=-1).movedim(-1, dim)


def model(sd, u, code, *, modes1, modes2, width, n_layers, s, iphi_sd, iphi_width, x_in=None, x_out=None, pre_trace=None):
    """sd: reference-layout state dict of one real dtype; u [B, N, in] -> [B, N, out].  pre_trace: a list that receives every
    feed-forward pre-activation [pixels, hidden] (the ReLU inputs), n_layers of them."""
    from oracle import ffno_oracle as orc
    F = torch.nn.functional
    dt = u.dtype
    x_in = u if x_in is None else x_in
    x_out = u if x_out is None else x_out
    xi_in = pmo.iphi(iphi_sd, x_in, code, iphi_width)
    xi_out = xi_in if x_out is x_in else pmo.iphi(iphi_sd, x_out, code, iphi_width)
    L, S, m1, m2 = n_layers, s, modes1, modes2

    def wy(i):
        return torch.view_as_complex(sd[f"convs.{i}.fourier_weight.0"])      # [W, W, m2]

    def wx(i):
        return torch.view_as_complex(sd[f"convs.{i}.fourier_weight.1"])      # [W, W, m1]

    def backcast(i, x_cf):
        """x_cf [B, W, S, S] -> backcast_ff_i on channels last -> [B, W, S, S]"""
        xs = x_cf.permute(0, 2, 3, 1)
        prefix = f"convs.{i}.backcast_ff."
        if pre_trace is not None:
            pre_trace.append(orc.linear_from_sd(sd, prefix + "layers.0.0.", xs).detach().reshape(-1, 2 * width))
        return orc.feedforward(sd, prefix, xs).permute(0, 3, 1, 2)

    h = F.linear(u, sd["fc0.weight"], sd["fc0.bias"]).permute(0, 2, 1) + 0j                        # [B, W, N]
    Oy = torch.einsum("bij,ioj->boj", torch.einsum("bcn,bnj->bcj", h, _modes_of(xi_in, 0, m2, -1)), wy(0))
    Ox = torch.einsum("bik,iok->bok", torch.einsum("bcn,bnk->bck", h, _modes_of(xi_in, 1, m1, -1)), wx(0))
    sep = _irfft_padded(Ox, S, -1)[:, :, :, None] + _irfft_padded(Oy, S, -1)[:, :, None, :]      # [B, W, x, y]
    G = torch.einsum("oi,ixy->oxy", sd["bs.0.weight"].reshape(width, 2), pmo.latent_grid(S, S, dt).to(u.device)) \
        + sd["bs.0.bias"][:, None, None]
    uc = backcast(0, sep) + G
    for i in range(1, L):
        xy = _irfft_padded(torch.einsum("bixy,ioy->boxy", torch.fft.rfft(uc, dim=-1)[..., :m2], wy(i)), S, -1)
        xx = _irfft_padded(torch.einsum("bixy,iox->boxy", torch.fft.rfft(uc, dim=-2)[:, :, :m1, :], wx(i)), S, -2)
        uc = uc + backcast(i, xx + xy) + G
    Ty = torch.einsum("bij,ioj->boj", torch.fft.rfft(uc.sum(dim=2), dim=-1)[..., :m2], wy(L))       # sum over x, transform in y
    Tx = torch.einsum("bik,iok->bok", torch.fft.rfft(uc.sum(dim=3), dim=-1)[..., :m1], wx(L))       # sum over y, transform in x
    t = torch.einsum("boj,bnj->bon", Ty, _modes_of(xi_out, 0, m2, 1)).real + torch.einsum("bok,bnk->bon", Tx, _modes_of(xi_out, 1, m1, 1)).real
    head = {"bs.weight": sd["bs.1.weight"].reshape(width, 2), "bs.bias": sd["bs.1.bias"], "fc1.weight": sd["fc1.weight"],
            "fc1.bias": sd["fc1.bias"], "fc2.weight": sd["fc2.weight"], "fc2.bias": sd["fc2.bias"]}
    return pmo.point_head(head, t, x_out)
