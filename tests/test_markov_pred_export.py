"""Grid2DMarkovExperiment with ``pred_path``: test_step's export of every prediction on the ``pred_size`` grid (reference
routines/grid_2d_markov.py:427-476) and ``write_predictions``, on the emulator and on the GPU.  The model, the data shapes and the
device routing are those of tests/test_markov_reduced_corr.py: one layer of width 32, three trajectories, four steps; the model
runs at 16 x 16 (f = 2) or 8 x 8 (f = 1, the reference's copy branch), pred_size = 8.  The oracle is tests/coarsen_oracle.py and
the numpy spectrum of tests/test_kernels_energy_spectrum.py, in float64, applied to the routine's OWN fp32 predictions.

Bounds, per rollout step (one velocity launch over the B images), in the L2 norm over the step's B images; u = 2^-24.
  vx, vy   The velocity launch is held to 1e-5 relative L2 per component (tests/test_velocity.py): |d u| <= 1e-5 |u|.  A block
           mean of f values of distinct cells shrinks an L2 error by sqrt(f) (Jensen).  The fp32 block mean adds f u max|u| per
           cell (tests/test_kernels_pred_export.py), sqrt(cells) times that in L2:
               |d vx| <= 1e-5 |u| / sqrt(f) + sqrt(B m m) f u max|u|,       f = 1: a copy, the first term alone.
  vort     f = 1: the prediction itself, bit for bit.  f > 1: each of the two differences doubles an inherited L2 error at most and
           divides it by the spacing, and the kernel's own arithmetic stays within 8 f u (max|v| / dx + max|u| / dy) per cell:
               |d w| <= 2 e-5 (|v| / dx + |u| / dy) / sqrt(f) + sqrt(B m m) 8 f u (max|v| / dx + max|u| / dy).
  spectrum E[s] = |P_s a|^2 / (2 m^2) with a = (vx, vy) of ONE image and P_s the orthogonal projector on shell s (Parseval).  For an
           error d of a:  |E[s](a + d) - E[s](a)| <= 2 sqrt(E[s]) e + e^2,  e = |d| / (sqrt(2) m)  -- quadratic, so twice the relative
           bound.  d is the error of the image's vx, vy (bounded by the step's whole L2 error above) plus that of the fp32 rfft2:
           at most 8 u log2(m) |a| per transformed dimension (Higham, Accuracy and Stability, theorem 24.2, eta about 7 u).  The
           summation adds (n + 11) u E[s] (tests/test_kernels_energy_spectrum.py).
"""
import os

import numpy as np
import pytest
import torch

import coarsen_oracle as co
from backend_util import host_device  # noqa: F401
from test_kernels_energy_spectrum import _lane_terms, spectrum64

B, M2, T, TC, N_STEPS, STEP = 3, 8, 6, 5, 4, 0.5
LX = LY = 2 * np.pi
U = 2.0 ** -24
VEL = 1e-5
KEYS = ("pred_vorticity", "pred_vx", "pred_vy", "pred_energy_spectrum")


def _routine(device, G, use_velocity, **kw):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    torch.manual_seed(5)
    blk = FNOFactorized2DBlock(modes=4, width=32, n_layers=1, input_dim=5 if use_velocity else 3, factor=2)
    exp = Grid2DMarkovExperiment(blk, n_steps=N_STEPS, step_size=STEP, grid_size=[G], use_velocity=use_velocity, noise_std=0.0,
                                 **kw).to(device)
    x = torch.from_numpy((np.random.RandomState(1).standard_normal((B, G, G, 1)) + 0.3).astype(np.float32)).to(device)
    exp.train()
    with torch.no_grad():
        exp._build_features({"x": x})      # the normaliser's statistics
    return exp.eval()


def _data(device, G, corr=False, times=True, n=B):
    rs = np.random.RandomState(2)
    batch = {"data": torch.from_numpy((rs.standard_normal((n, G, G, T)) + 0.3).astype(np.float32)).to(device)}
    if times:
        batch["times"] = torch.from_numpy(np.tile(np.arange(T, dtype=np.float32) * STEP, (n, 1))).to(device)
    if corr:
        batch["corr_data"] = torch.from_numpy((rs.standard_normal((n, M2, M2, TC)) + 0.2).astype(np.float32)).to(device)
    return batch


def _same(a, b, keys):
    for k in keys:
        if torch.is_tensor(a[k]):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
        else:
            assert a[k] == b[k], k


def _norm(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


@pytest.mark.parametrize("G,kw", [(16, dict(use_velocity=True)), (16, dict(use_velocity=False, downsample_corr=True)),
                                  (8, dict(use_velocity=True))])
def test_exported_arrays_match_the_oracle_and_the_metrics_do_not_move(host_device, G, kw):
    corr = bool(kw.get("downsample_corr"))
    exp = _routine(host_device, G, pred_path="out/preds.nc", pred_size=M2, **kw)
    plain = _routine(host_device, G, **kw)
    batch = _data(host_device, G, corr=corr)
    out, base = exp.test_step(batch), plain.test_step(batch)
    assert set(out) == set(base) | set(KEYS) and not set(KEYS) & set(base)
    _same(out, base, base)      # every metric bit for bit, the shared velocity image included
    assert out["test_correlations"].shape == (N_STEPS,) and ("corr_data" in batch) == corr
    preds = exp._traj[0].cpu().numpy()
    assert preds.tobytes() == plain._traj[0].cpu().numpy().tobytes()
    m, f = M2, G // M2
    got = {k: out[k].cpu().numpy().astype(np.float64) for k in KEYS}
    for k in KEYS[:3]:
        assert out[k].shape == (N_STEPS, B, m, m) and out[k].device.type == torch.device(host_device).type
    assert out[KEYS[3]].shape == (N_STEPS, B, m // 2 + 1)
    dx, dy, cells = LX / m, LY / m, np.sqrt(B * m * m)
    terms = _lane_terms(m)
    for t in range(N_STEPS):
        w = preds[..., t]
        u, v = co.velocity(w, LX, LY)
        if f == 1:
            u_c, v_c, w_c = u, v, w.astype(np.float64)
            b_x, b_y = VEL * _norm(u), VEL * _norm(v)
            assert out["pred_vorticity"][t].cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes()
        else:
            u_c, v_c = co.coarsen_velocity(u, v, m)
            w_c = co.curl(u_c, v_c, LX, LY)
            b_x = VEL * _norm(u) / np.sqrt(f) + cells * f * U * np.abs(u).max()
            b_y = VEL * _norm(v) / np.sqrt(f) + cells * f * U * np.abs(v).max()
            b_w = 2 * VEL * (_norm(v) / dx + _norm(u) / dy) / np.sqrt(f) + cells * 8 * f * U * (np.abs(v).max() / dx + np.abs(u).max() / dy)
            e_w = _norm(got["pred_vorticity"][t] - w_c)
            print(f"G={G} t={t}: |d vort| {e_w:.3e}, bound {b_w:.3e}")
            assert e_w <= b_w
        e_x, e_y = _norm(got["pred_vx"][t] - u_c), _norm(got["pred_vy"][t] - v_c)
        print(f"G={G} t={t}: |d vx| {e_x:.3e} (bound {b_x:.3e}), |d vy| {e_y:.3e} (bound {b_y:.3e})")
        assert e_x <= b_x and e_y <= b_y
        E = spectrum64(np.fft.rfft2(u_c), np.fft.rfft2(v_c))
        for b in range(B):
            d = np.hypot(b_x, b_y) + 2 * 8 * U * np.log2(m) * np.hypot(_norm(u_c[b]), _norm(v_c[b]))
            e = d / (np.sqrt(2) * m)
            bound = 2 * np.sqrt(E[b]) * e + e * e + (terms + 11) * U * E[b]
            err = np.abs(got["pred_energy_spectrum"][t, b] - E[b])
            if b == 0:
                print(f"G={G} t={t}: max spectrum err / bound {np.max(err / bound):.3f}")
            assert (err <= bound).all()
    # the public function on the exported slabs takes the same launch: the same bits
    from fourierflow_amd import diagnostics
    again = diagnostics.energy_spectrum(out["pred_vx"], out["pred_vy"])
    assert again.cpu().numpy().tobytes() == out["pred_energy_spectrum"].cpu().numpy().tobytes()


def test_validation_never_exports(host_device):
    from fourierflow_amd import _lib
    exp = _routine(host_device, 16, True, pred_path="out/preds.nc", pred_size=M2)
    batch = _data(host_device, 16)
    lib, calls = _lib.get_lib(), []
    names = ("ffno_prediction_export_step", "ffno_energy_spectrum")
    saved = {n: getattr(lib, n) for n in names}
    for n in names:
        setattr(lib, n, lambda *a, _f=saved[n], _n=n: (calls.append(_n), _f(*a))[1])
    try:
        v = exp.validation_step(batch)
        assert not [k for k in v if k.startswith("pred_")] and calls == [] and exp._pred is None
        t = exp.test_step(batch)
        assert set(KEYS) <= set(t) and calls == [names[0]] * N_STEPS + [names[1]]      # one launch per step, one after the loop
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)


def test_write_predictions_round_trip_of_two_batches(host_device, tmp_path):
    exp = _routine(host_device, 16, True, pred_path=str(tmp_path / "deep" / "er" / "preds.nc"), pred_size=M2,
                   domain=((0.0, LX), (1.0, 3.0)))
    first, second = _data(host_device, 16), _data(host_device, 16, n=2)
    parts = [exp.test_step(first), exp.test_step(second)]
    written = exp.write_predictions(None, parts, parts[0]["test_times"])
    assert written == str(tmp_path / "deep" / "er" / "preds.npz") and os.listdir(tmp_path / "deep" / "er") == ["preds.npz"]
    with np.load(written) as z:
        assert set(z.files) == {"vorticity", "vx", "vy", "time", "x", "y", "energy_spectrum", "k"}
        for name, key in (("vorticity", KEYS[0]), ("vx", KEYS[1]), ("vy", KEYS[2])):
            a = z[name]
            assert a.shape == (B + 2, M2, M2, N_STEPS) and a.dtype == np.float32
            for lo, p in ((0, parts[0]), (B, parts[1])):      # [sample, x, y, time] from the time-major slabs, batch after batch
                want = p[key].cpu().numpy()
                assert np.array_equal(a[lo:lo + want.shape[1]], np.transpose(want, (1, 2, 3, 0)))
        assert z["energy_spectrum"].shape == (B + 2, N_STEPS, M2 // 2 + 1)
        assert np.array_equal(z["energy_spectrum"][B:], np.transpose(parts[1][KEYS[3]].cpu().numpy(), (1, 0, 2)))
        assert np.array_equal(z["time"], np.arange(T - N_STEPS, T, dtype=np.float32) * STEP)
        np.testing.assert_allclose(z["x"], (np.arange(M2) + 0.5) * LX / M2, rtol=1e-15)
        np.testing.assert_allclose(z["y"], 1.0 + (np.arange(M2) + 0.5) * 2.0 / M2, rtol=1e-15)
        assert np.array_equal(z["k"], np.arange(M2 // 2 + 1))
    # no `times` in the batch: step_size * (1 .. n_steps); another path, given explicitly, a name without .nc is kept
    part = exp.test_step(_data(host_device, 16, times=False))
    assert "test_times" not in part
    other = exp.write_predictions(str(tmp_path / "p.npz"), [part])
    assert other == str(tmp_path / "p.npz")
    with np.load(other) as z:
        assert np.array_equal(z["time"], STEP * np.arange(1, N_STEPS + 1)) and z["vx"].shape == (B, M2, M2, N_STEPS)
    with pytest.raises(ValueError, match="pred_vorticity"):
        exp.write_predictions(None, [{"test_loss": 0.0}])


@pytest.mark.parametrize("size", [7, 9, 4, 512, 0])
def test_a_pred_size_the_spectrum_cannot_take_is_refused_at_construction(size):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    blk = FNOFactorized2DBlock(modes=4, width=32, n_layers=1, input_dim=3, factor=2)
    with pytest.raises(ValueError, match=f"pred_size.*{size}"):
        Grid2DMarkovExperiment(blk, n_steps=N_STEPS, grid_size=[16], pred_path="preds.nc", pred_size=size)
    assert Grid2DMarkovExperiment(blk, n_steps=N_STEPS, grid_size=[16]).pred_size == 64      # the reference's hard-coded grid


def test_a_model_grid_that_is_no_multiple_of_pred_size_is_refused_at_the_first_batch(host_device):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    blk = FNOFactorized2DBlock(modes=4, width=32, n_layers=1, input_dim=3, factor=2)
    exp = Grid2DMarkovExperiment(blk, n_steps=N_STEPS, grid_size=[12], pred_path="preds.nc", pred_size=M2).to(host_device).eval()
    with pytest.raises(ValueError) as e:
        exp.test_step(_data(host_device, 12))
    for word in ("12 x 12", "8 x 8", "pred_size=8", "12 / 8"):
        assert word in str(e.value), (word, str(e.value))
