"""Grid2DMarkovExperiment fed by MultiResolutionMarkovData (builders/markov_data.py): the engine changes its geometry between
consecutive optimiser steps -- 8 x 8 / 16 x 16 on the emulator (width 32, 4 modes), 32 x 32 / 64 x 64 on the GPU (width 64, 16 modes:
at 32 x 32 every bin but Nyquist, the edge of the shipped multi_resolution configs) -- two layers, use_velocity, batches of 4.

22 pairs (n = 2, T = 13, k = 2) in batches of 4: five full batches and one of 2; with one loader worker the sets alternate 0 1 0 1 0 1,
so an epoch sees the geometries (4, set 0), (4, set 1) and (2, set 1).  Epoch 0 accumulates the normaliser statistics, epochs 1 and 2
take six optimiser steps each.

The run through the new set is compared, bit for bit, with
    the control          one routine fed batches drawn by hand with single-size MarkovTrajectoryData.gather calls in the same order
    the separated run    two routines, one per grid size, each of which sees only its own size's steps; the whole training state
                         (parameters, normaliser, AdamW moments, step counters) is handed across after every step.  Nothing that
                         an engine keeps between steps can have come from the other size there.
Everything is computed once per device and shared by the tests below."""
import numpy as np
import torch

import golden_util as gu
from backend_util import host_device, rel_l2  # noqa: F401

N_TRAJ, T, K, B, SEED = 2, 13, 2, 4, 3
PAIRS = N_TRAJ * (T - K)
BATCHES = -(-PAIRS // B)
assert (PAIRS, BATCHES, PAIRS % B) == (22, 6, 2)
STATS = ("sum", "sum_squared", "count", "n_accumulations")


def _geometry(device):
    return dict(width=32, modes=4, sizes=(8, 16)) if device == "cpu" else dict(width=64, modes=16, sizes=(32, 64))


def _arrays(sizes):
    rs = np.random.RandomState(41)
    return [(rs.standard_normal((N_TRAJ, g, g, T)) + 0.3).astype(np.float32) for g in sizes]


def _routine(device, g):
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    torch.manual_seed(11)
    conv = FNOFactorized2DBlock(modes=g["modes"], width=g["width"], input_dim=5, n_layers=2, share_weight=True, factor=4,
                                ff_weight_norm=True, gain=0.1)
    return Grid2DMarkovExperiment(conv, use_velocity=True, grid_size=list(g["sizes"]), max_accumulations=1000, noise_std=0.0,
                                  optimizer=dict(lr=2.5e-3, weight_decay=1e-4),
                                  scheduler=dict(num_warmup_steps=3, num_training_steps=40, num_cycles=0.5)).to(device)


def _state(routine):
    return {k: v.detach().cpu().numpy().copy() for k, v in routine.state_dict().items()}


def _hand_over(src, dst):
    """The whole training state of `src` into `dst`."""
    dst.load_state_dict(src.state_dict())
    a, b = src.trainer(), dst.trainer()
    b.m.copy_(a.m)
    b.v.copy_(a.v)
    b.step_count, b.opt_step = a.step_count, a.opt_step


def _steps(routines, epoch, batches, after=None):
    """One epoch: batch i goes to routines[set of batch i] -> the losses (none in epoch 0), each read before the next step: the
    routine returns the trainer's one loss buffer."""
    losses = []
    for s, batch in batches:
        loss = routines[s].training_step(batch, epoch=epoch)
        assert (loss is None) == (epoch == 0)
        if loss is not None:
            losses.append(float(loss.item()))
        if after is not None:
            after(s)
    return losses


def _hand_drawn(singles, device, epochs):
    """The batches of `epochs` epochs drawn with single-size gather calls: the permutation stream of seed SEED, batch i from set
    i % 2."""
    gen, out = torch.Generator().manual_seed(SEED), []
    for _ in range(epochs):
        ids = torch.randperm(PAIRS, generator=gen).to(torch.int32).to(device)
        out.append([(i % 2, singles[i % 2].gather(ids, i * B, min(B, PAIRS - i * B))) for i in range(BATCHES)])
    return out


_RUNS = {}


def _runs(device):
    if device in _RUNS:
        return _RUNS[device]
    from fourierflow_amd.builders import MarkovTrajectoryData, MultiResolutionMarkovData
    g = _geometry(device)
    arrays = _arrays(g["sizes"])
    out = {}

    # ---- the run through the new set: statistics, six steps, [validation-shaped passes, six more steps] twice ------------------
    data = MultiResolutionMarkovData(arrays, device=device, batch_size=B, k=K, num_workers=1, seed=SEED)
    singles = [MarkovTrajectoryData(a, device=device, batch_size=B, mode="kolmogorov", k=K, seed=0, shuffle=False) for a in arrays]
    held = torch.arange(PAIRS, dtype=torch.int32).to(device)
    valid = [singles[1].gather(held, 0, 3), singles[1].gather(held, 3, 1)]      # a full and a short validation batch
    r = _routine(device, g)
    eng = r.trainer().engine
    sets, shapes = [], []

    def epoch_batches():
        batches = [(data.set_index(i), b) for i, b in enumerate(data.epoch())]
        sets.append([s for s, _ in batches])
        shapes.append([tuple(b["x"].shape) for _, b in batches])
        return batches

    def validate():
        r.eval()
        losses = [r.pair_loss(b) for b in valid]
        r.train()
        return losses

    _steps([r, r], 0, epoch_batches())
    out["multi_stats"] = {k: v for k, v in _state(r).items() if k.startswith("normalizer.")}
    losses = _steps([r, r], 1, epoch_batches())
    out["multi_state6"] = _state(r)
    validate()
    seen = dict(eng._ws_cache)                              # every geometry of the run has been seen once by now
    losses += _steps([r, r], 2, epoch_batches())
    validate()
    out["cache_first"], out["cache_last"] = seen, dict(eng._ws_cache)
    out["multi_losses"] = losses
    out["sets"], out["shapes"] = sets, shapes

    # ---- the control: the same batches drawn by hand, no validation passes in between ------------------------------------------
    for name in ("control", "control_again"):
        c = _routine(device, g)
        drawn = _hand_drawn(singles, device, 2)
        _steps([c, c], 0, drawn[0])
        out[name + "_stats"] = {k: v for k, v in _state(c).items() if k.startswith("normalizer.")}
        out[name + "_losses"] = _steps([c, c], 1, drawn[1])
        out[name + "_state6"] = _state(c)

    # ---- the separated run: one routine per size, the training state handed across after every step ---------------------------
    pair = [_routine(device, g), _routine(device, g)]
    drawn = _hand_drawn(singles, device, 2)
    _steps(pair, 0, drawn[0], after=lambda s: _hand_over(pair[s], pair[1 - s]))
    out["separated_losses"] = _steps(pair, 1, drawn[1], after=lambda s: _hand_over(pair[s], pair[1 - s]))
    out["separated_geometries"] = [{k[:2] for k in p.trainer().engine._ws_cache} for p in pair]
    _RUNS[device] = out
    return out


def _worst(a, b):
    return max(float(np.max(np.abs(a[k].astype(np.complex128) - b[k].astype(np.complex128)))) for k in a)


def _repeatability(run):
    """Twice the control's own run-to-run difference (0.0 where the control repeats itself bit for bit): (losses, state)."""
    dl = max(abs(a - b) for a, b in zip(run["control_losses"], run["control_again_losses"]))
    return 2 * dl, 2 * _worst(run["control_state6"], run["control_again_state6"])


def test_the_run_alternates_sizes_every_step(host_device):
    run, g = _runs(host_device), _geometry(host_device)
    a, b = g["sizes"]
    assert run["sets"] == [[0, 1, 0, 1, 0, 1]] * 3
    assert run["shapes"] == [[(4, a, a, 1), (4, b, b, 1), (4, a, a, 1), (4, b, b, 1), (4, a, a, 1), (2, b, b, 1)]] * 3
    assert len(run["multi_losses"]) == 12 and all(np.isfinite(run["multi_losses"]))


def test_statistics_epoch_equals_the_hand_drawn_control(host_device):
    """(a) sum / sum_squared / count of the normaliser after epoch 0 over all batches, both sizes."""
    run = _runs(host_device)
    for k in STATS:
        got, want = run["multi_stats"]["normalizer." + k], run["control_stats"]["normalizer." + k]
        print(f"[multi-resolution {host_device}] normalizer.{k}: {got.ravel()[:5]} vs control {want.ravel()[:5]}")
        assert got.tobytes() == want.tobytes(), k
    assert float(run["multi_stats"]["normalizer.n_accumulations"]) == BATCHES
    g = _geometry(host_device)
    assert float(run["multi_stats"]["normalizer.count"]) == sum(4 * s * s for s in g["sizes"]) * 2 + 4 * g["sizes"][0] ** 2 + \
        2 * g["sizes"][1] ** 2


def test_six_steps_equal_the_hand_drawn_control(host_device):
    """(b) the losses of six optimiser steps and the parameters after them."""
    run = _runs(host_device)
    tol_l, tol_s = _repeatability(run)
    dl = max(abs(a - b) for a, b in zip(run["multi_losses"][:6], run["control_losses"]))
    ds = _worst(run["multi_state6"], run["control_state6"])
    print(f"[multi-resolution {host_device}] vs control: losses differ by {dl:.3g}, state by {ds:.3g}; twice the control's own "
          f"run-to-run difference: {tol_l:.3g} / {tol_s:.3g}")
    assert set(run["multi_state6"]) == set(run["control_state6"]) and len(run["multi_state6"]) > 10
    assert dl <= tol_l and ds <= tol_s


def test_no_state_leaks_across_a_shape_switch(host_device):
    """(c) the same losses as two routines that each see only their own size's steps."""
    run, g = _runs(host_device), _geometry(host_device)
    assert run["separated_geometries"] == [{(4, (s, s)), (2, (s, s))} if i else {(4, (s, s))} for i, s in enumerate(g["sizes"])]
    tol_l, _ = _repeatability(run)
    dl = max(abs(a - b) for a, b in zip(run["multi_losses"][:6], run["separated_losses"]))
    print(f"[multi-resolution {host_device}] vs separated routines: losses differ by {dl:.3g} (bound {tol_l:.3g}): "
          f"{run['multi_losses'][:6]} / {run['separated_losses']}")
    assert len(run["separated_losses"]) == 6 and dl <= tol_l


def test_steady_state_allocates_no_workspace(host_device):
    """(e) after the first batch of each geometry -- the full training batch of either size, the short one, the full and the short
    validation batch -- the engine's cache holds the same workspace objects after step 12 as after step 6."""
    run = _runs(host_device)
    first, last = run["cache_first"], run["cache_last"]
    a, b = _geometry(host_device)["sizes"]
    want = {(4, (a, a), True), (4, (b, b), True), (2, (b, b), True), (3, (b, b), False), (1, (b, b), False)}
    assert {k[:3] for k in first} == want, sorted(k[:3] for k in first)
    assert set(last) == set(first) and len(last) == 5
    assert all(last[k] is first[k] for k in first)


def test_forward_at_every_bin_but_nyquist_matches_the_oracle(host_device):
    """(d) 32 x 32 with 16 modes at width 64: the bound of tests/test_block.py."""
    import oracle_util as ou
    from test_block import build_block
    kw = dict(modes=16, width=64, input_dim=5, n_layers=2, share_weight=True, factor=4, ff_weight_norm=True, gain=0.1)
    seed, nb = 21, 2
    blk = build_block(kw, seed, host_device)
    x_np, _ = gu.make_block_io(kw, seed, nb, 32, 32)
    ref = ou.oracle_block_run(kw, seed, nb, 32, 32)[0]["forecast"].detach().numpy()
    x = torch.from_numpy(x_np).to(host_device)
    saving = blk(x)["forecast"].detach()              # the training forward (it saves for a backward pass) ...
    with torch.no_grad():
        plain = blk(x)["forecast"]                    # ... and the inference forward
    for name, pred in (("training", saving), ("inference", plain)):
        err = rel_l2(pred.cpu().numpy(), ref)
        print(f"[multi-resolution {host_device}] {name} forward 32 x 32, 16 modes, width 64 vs oracle: rel L2 {err:.3g}")
        assert err < 1e-5, name
