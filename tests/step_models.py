"""Plain numpy models of the step kernels, written from the formulas and not from the kernel sources' helpers:

  adam_model   torch.optim.AdamW (decoupled decay) / torch.optim.Adam (L2 decay joins the gradient) in the dtype it is given --
               np.float64 is the reference of tests/test_kernels_step.py, np.float32 its rounding floor
  keep_model   the dropout keep set of (seed, p, n): fmix32(fmix32(idx + fmix32(seed)) ^ fmix32(~seed)) >= thr in uint64
               arithmetic masked to 32 bits (fmix32 = the 32-bit murmur3 finaliser)
"""
import numpy as np

TERMS = ("decay", "grad_scale", "bc1", "bc2", "eps")     # what `without` can leave out of adam_model


def f32(x):
    """A scalar argument as the C ABI receives it: rounded to fp32, held as a Python float."""
    return float(np.float32(x))


def adam_model(p, g, m, v, step, lr, beta1, beta2, eps, wd, grad_scale, decoupled, dtype=np.float64, without=None):
    """One optimiser step -> (p, m, v).  `without` leaves one term out: "decay" (no weight decay of either kind), "grad_scale"
    (taken as 1), "bc1" / "bc2" (bias correction frozen at its step-3 value), "eps" (taken as 0)."""
    assert without is None or without in TERMS
    T = dtype
    p, g, m, v = (np.asarray(a, T) for a in (p, g, m, v))
    lr, beta1, beta2, eps, wd, grad_scale = (T(f32(s)) for s in (lr, beta1, beta2, eps, wd, grad_scale))
    one = T(1)
    if without == "decay":
        wd = T(0)
    if without == "grad_scale":
        grad_scale = one
    if without == "eps":
        eps = T(0)
    g = g * grad_scale
    if decoupled:
        p = p * (one - lr * wd)
    else:
        g = g + wd * p
    m = beta1 * m + (one - beta1) * g
    v = beta2 * v + (one - beta2) * g * g
    bc1 = one - beta1 ** T(3 if without == "bc1" else step)
    bc2 = one - beta2 ** T(3 if without == "bc2" else step)
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p.astype(T), m.astype(T), v.astype(T)


_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = np.asarray(h, np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h = h ^ (h >> np.uint64(16))
    return h


def keep_threshold(p):
    return min(2 ** 32 - 1, int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32)))


def keep_model(n, p, seed):
    """-> bool[n]: element idx is kept iff its hash is >= thr = min(2^32 - 1, floor(float32(p) 2^32))."""
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    idx = np.arange(n, dtype=np.uint64)
    k1, k2 = _fmix32(seed), _fmix32(~seed & _M32)
    h = _fmix32(_fmix32((idx + k1) & _M32) ^ k2)
    return h >= np.uint64(keep_threshold(p))
