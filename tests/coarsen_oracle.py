"""float64 numpy restatement of the reference's reduction of a vorticity image to the grid of ``corr_data`` and of the
correlation taken there (utils/array.py:18-80 ``downsample_vorticity``, routines/grid_2d_markov.py:350-370).  jax-cfd is not
installed, so no golden of the reference itself exists; tests/test_kernels_coarsen.py pins this restatement by a closed form.

    velocity(w)                       (u, v) of a vorticity image through the stream function (the formula of :130-144)
    coarsen_velocity(u, v, m)         jax-cfd's downsample_staggered_velocity: for each component every f-th line along its own
                                      direction, the LAST of each block, and the mean over blocks of f across it
    curl(u_c, v_c, lx, ly)            velocity_to_vorticity: forward differences with periodic wrap, dx = lx / m, dy = ly / m
    coarsen_from_velocity(vel, ...)   the two above on a [..., X, Y, 3] velocity-feature image (what the kernel reads)
    downsample_vorticity(w, m, ...)   the whole chain on [B, X, Y, T]
    correlation(wc, corr, n_steps)    p_2 [n_steps], diverged index
"""
import numpy as np


def velocity(w, lx=2 * np.pi, ly=2 * np.pi):
    """w [..., X, Y] -> (u, v), float64: psi^ = -w^ / lap, u = psi_y, v = -psi_x."""
    w = np.asarray(w, np.float64)
    X, Y = w.shape[-2:]
    kx = np.fft.fftfreq(X, d=lx / X)[:, None]
    ky = np.fft.rfftfreq(Y, d=ly / Y)[None, :]
    lap = (2j * np.pi) ** 2 * (kx ** 2 + ky ** 2)
    lap[0, 0] = 1
    psi = -np.fft.rfftn(w, axes=(-2, -1)) / lap
    u = np.fft.irfftn(2j * np.pi * ky * psi, s=(X, Y), axes=(-2, -1))
    v = np.fft.irfftn(-2j * np.pi * kx * psi, s=(X, Y), axes=(-2, -1))
    return u, v


def coarsen_velocity(u, v, m):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    X, Y = u.shape[-2:]
    f = X // m
    assert X == f * m and Y == f * m, (X, Y, m)
    lead = u.shape[:-2]
    u_c = u.reshape(*lead, m, f, m, f)[..., :, f - 1, :, :].mean(axis=-1)
    v_c = v.reshape(*lead, m, f, m, f)[..., :, :, :, f - 1].mean(axis=-2)
    return u_c, v_c


def curl(u_c, v_c, lx=2 * np.pi, ly=2 * np.pi):
    m = u_c.shape[-1]
    dx, dy = np.float64(lx) / m, np.float64(ly) / m
    return (np.roll(v_c, -1, axis=-2) - v_c) / dx - (np.roll(u_c, -1, axis=-1) - u_c) / dy


def coarsen_from_velocity(vel, m, lx=2 * np.pi, ly=2 * np.pi):
    """vel [..., X, Y, 3] (vorticity, u, v) -> w_c [..., m, m]."""
    vel = np.asarray(vel, np.float64)
    return curl(*coarsen_velocity(vel[..., 1], vel[..., 2], m), lx, ly)


def downsample_vorticity(w, m, lx=2 * np.pi, ly=2 * np.pi):
    """w [B, X, Y, T] -> [B, m, m, T]."""
    wt = np.moveaxis(np.asarray(w, np.float64), -1, 1)
    u, v = velocity(wt, lx, ly)
    return np.moveaxis(curl(*coarsen_velocity(u, v, m), lx, ly), 1, -1)


def correlation(wc, corr, n_steps, threshold=0.95):
    """wc [B, m, m, n_steps], corr [B, m, m, Tc] -> (p_2 [n_steps], diverged index)."""
    wc, c = np.asarray(wc, np.float64), np.asarray(corr, np.float64)[..., -n_steps:]
    nrm = lambda a: np.sqrt((a ** 2).sum(axis=(1, 2)))      # noqa: E731
    p = ((wc * c).sum(axis=(1, 2)) / (nrm(wc) * nrm(c))).mean(axis=0)
    below = np.nonzero(p < threshold)[0]
    return p, int(below[0]) if len(below) else n_steps
