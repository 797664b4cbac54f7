"""float64 numpy restatement of the Kolmogorov-flow generator's solver for the tests, written from the formulas in the FULL complex
form (every transform an N x N complex FFT, the physical fields the real parts of the inverse transforms -- which drops a
derivative along an axis at that axis' Nyquist bin, what the half-spectrum kernels of csrc/ffno_kf2d.h reproduce by writing zeros):

    vorticity equation   w_t + v . grad(w) = nu lap(w) - drag w + c w + f     on the periodic square [0, len)^2
    v = (psi_y, -psi_x), psi_h = w_h / |k|^2 (0 at k = 0);   f(y_j) = -magnitude k_f cos(k_f y_j), y_j = (j + 1/2) len / N
    explicit part   E(w_h) = -filt fft2(v_x w_x + v_y w_y) + c w_h + f_h,   filt: 9 (i_x^2 + i_y^2) <= N^2 in bin indices
    implicit part   L = -nu |k|^2 - drag
    one step        Carpenter-Kennedy low-storage RK4(5) for E with Crank-Nicolson for L: for s = 0..4
                        h <- E(w_h) + beta_s h;   w_h <- (w_h + gamma_s dt h + mu_s L w_h) / (1 - mu_s L),   mu_s = dt (a_{s+1} - a_s) / 2

The coefficients are restated here (not imported from the package), so a typing slip on either side shows.  The reduction to a
coarse grid is tests/coarsen_oracle.py's.
"""
import numpy as np

import coarsen_oracle as co

ALPHA = [0, 0.1496590219993, 0.3704009573644, 0.6222557631345, 0.9582821306748, 1]
BETA = [0, -0.4178904745, -1.192151694643, -1.697784692471, -1.514183444257]
GAMMA = [0.1496590219993, 0.3792103129999, 0.8229550293869, 0.6994504559488, 0.1530572479681]


def indices(N):
    i = np.fft.fftfreq(N, 1.0 / N)      # 0 .. N/2-1, -N/2 .. -1
    return i[:, None], i[None, :]


def force_field(N, wavenumber, magnitude, length=2 * np.pi):
    """f [N, N]: -magnitude k cos(k y_j) with y along axis 1, sampled at the cell centres."""
    y = (np.arange(N) + 0.5) * length / N
    return np.broadcast_to(-magnitude * wavenumber * np.cos(wavenumber * y)[None, :], (N, N)).copy()


class Solver:
    def __init__(self, N, viscosity, drag, dt, wavenumber=0, magnitude=0.0, linear_coefficient=0.0, length=2 * np.pi,
                 explicit_only=False):
        ix, iy = indices(N)
        k0 = 2 * np.pi / length
        self.N, self.dt, self.c = N, float(dt), float(linear_coefficient)
        self.kx, self.ky = k0 * ix, k0 * iy
        self.k2 = self.kx ** 2 + self.ky ** 2
        self.inv = np.where(self.k2 > 0, 1.0 / np.where(self.k2 > 0, self.k2, 1.0), 0.0)
        self.filt = (9 * (ix ** 2 + iy ** 2) <= N * N).astype(np.float64)
        self.L = np.zeros_like(self.k2) if explicit_only else -viscosity * self.k2 - drag
        self.f_h = np.fft.fft2(force_field(N, wavenumber, magnitude, length)) if magnitude and wavenumber else 0.0

    def velocity(self, w_h):
        psi = w_h * self.inv
        return np.fft.ifft2(1j * self.ky * psi).real, np.fft.ifft2(-1j * self.kx * psi).real

    def explicit(self, w_h):
        vx, vy = self.velocity(w_h)
        w_x, w_y = np.fft.ifft2(1j * self.kx * w_h).real, np.fft.ifft2(1j * self.ky * w_h).real
        return -self.filt * np.fft.fft2(vx * w_x + vy * w_y) + self.c * w_h + self.f_h

    def step(self, w_h):
        h = 0.0
        for s in range(5):
            h = self.explicit(w_h) + BETA[s] * h
            mu = 0.5 * self.dt * (ALPHA[s + 1] - ALPHA[s])
            w_h = (w_h + GAMMA[s] * self.dt * h + mu * self.L * w_h) / (1 - mu * self.L)
        return w_h

    def run(self, w0, n_steps):
        """w0 [..., N, N] real -> the field after n_steps, real."""
        w_h = np.fft.fft2(np.asarray(w0, np.float64))
        for _ in range(n_steps):
            w_h = self.step(w_h)
        return np.fft.ifft2(w_h).real

    def downsample(self, w, m, length=2 * np.pi):
        """w [..., N, N] -> [..., m, m]: the staggered-velocity reduction; m = N: w itself."""
        if m == self.N:
            return np.asarray(w, np.float64)
        vx, vy = self.velocity(np.fft.fft2(np.asarray(w, np.float64)))
        return co.curl(*co.coarsen_velocity(vx, vy, m), length, length)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
