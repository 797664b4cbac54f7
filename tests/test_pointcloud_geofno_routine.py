"""PointCloudExperiment with the geo-FNO baseline (FNOPointCloud2D + IPhi, torch.optim.Adam + StepLR per epoch): three Adam
steps (lr 1e-3, weight decay 1e-4) follow float64 autograd through the restatement of tests/pointcloud_geofno_oracle.py +
torch.optim.Adam (loss within 1e-5 per step, every parameter <= 1e-5 rel-L2 afterwards: the bands of the same test in
tests/test_geofno.py); StepLR moves with the epoch counter; model.ws.* is trained, iphi.fc_no_code.* is never written; a
checkpoint resumes bit for bit; the F-FNO model keeps AdamW with the cosine schedule.

Conditioning of the Adam comparison.  The reference initialises the Fourier weights at 1 / W^2 x U[0, 1) ~ 5e-4, below the
learning rate: three Adam steps of ~1e-3 each replace such a weight, so its relative error afterwards IS the relative error of
m / (sqrt(v) + eps), which fp32 rounding of the gradient moves by far more than 1e-5 wherever |g| is near eps = 1e-8 (lr / eps =
1e5).  That is a property of Adam in fp32, not of any kernel: the restatement itself, run in float32 under torch.optim.Adam, ends
1.3e-4 from its float64 run at the reference's initial scale (3.5e-5 with the Fourier weights x 10, 5.3e-6 x 30, 2.3e-6 x 100;
measured on the CPU, no kernel involved).  So the test scales the Fourier weights by 100 (|w| ~ 0.05, the magnitude of a trained
layer), and first asserts ON THE RESTATEMENT ALONE that its float32 run stays within a third of both bands."""
import numpy as np
import torch

import pointcloud_geofno_oracle as pgo
import pointcloud_model_oracle as pmo
from backend_util import host_device, rel_l2  # noqa: F401  (host_device is a fixture)

B, W, M1, M2, S1, S2, N, L = 2, 32, 3, 2, 8, 10, 37, 3
OPT = dict(lr=1e-3, weight_decay=1e-4)
SCH = dict(step_size=2, gamma=0.5)
FOURIER_SCALE = 100.0      # see the module docstring
LOSS_TOL = PARAM_TOL = 1e-5


def _routine(seed):
    from fourierflow_amd.modules import FNOPointCloud2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    torch.manual_seed(seed)
    model = FNOPointCloud2D(M1, M2, W, 2, 1, n_layers=L, s1=S1, s2=S2)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".weights" in n:
                p.mul_(FOURIER_SCALE)
    return PointCloudExperiment(model, IPhi(16), 10, optimizer=dict(OPT), scheduler=dict(SCH), optimizer_type="adam")


def _batches(n_steps, seed):
    rng = np.random.default_rng(seed)
    return [dict(xy=rng.uniform(0.05, 0.95, (B, N, 2)).astype(np.float32), rr=rng.standard_normal((B, 42)).astype(np.float32),
                 sigma=rng.standard_normal((B, N, 1)).astype(np.float32)) for _ in range(n_steps)]


def _oracle_training(routine, batches, dtype=torch.float64):
    sd, uniq = pmo.model_state_dict(routine.model.state_dict(), dtype)
    isd, iuniq = pmo.model_state_dict(routine.iphi.state_dict(), dtype)
    opt = torch.optim.Adam(list(uniq.values()) + list(iuniq.values()), **OPT)
    losses = []
    for b in batches:
        t = {k: torch.tensor(v, dtype=dtype) for k, v in b.items()}
        out = pgo.model(sd, t["xy"], t["rr"], iphi_sd=isd, iphi_width=routine.iphi.width, modes1=M1, modes2=M2, width=W,
                        n_layers=L, s1=S1, s2=S2)
        loss = pmo.rel_l2_loss(out, t["sigma"])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    final = {"model." + k: v for k, v in uniq.items()}
    final.update({"iphi." + k: v for k, v in iuniq.items()})
    return losses, {k: (torch.view_as_real(v) if v.is_complex() else v).detach().numpy() for k, v in final.items()}


def test_three_adam_steps_follow_the_oracle(host_device, tmp_path):
    routine = _routine(40)
    batches = _batches(4, 41)
    ref_losses, ref_final = _oracle_training(routine, batches[:3])
    # precondition, on the restatement alone: its own float32 run holds a third of both bands
    l32, f32 = _oracle_training(routine, batches[:3], torch.float32)
    noise_l = max(abs(a - b) for a, b in zip(l32, ref_losses))
    noise_p = max(rel_l2(f32[k], ref_final[k]) for k in ref_final if not k.startswith("iphi.fc_no_code."))
    print(f"float32 restatement vs float64: loss {noise_l:.2e}, worst parameter {noise_p:.2e}")
    assert noise_l <= LOSS_TOL / 3 and noise_p <= PARAM_TOL / 3
    init = {k: v.detach().clone() for k, v in routine.named_parameters()}
    routine.to(host_device)
    dev = lambda b: {k: torch.tensor(v, device=host_device) for k, v in b.items()}      # noqa: E731

    tr = routine.trainer()
    assert tr.decoupled is False and tr.lr_factor is not None
    names = list(tr.engine.param_names)
    assert [n for n in names if n.startswith("model.ws.")] == [f"model.ws.{i}.{p}" for i in range(L - 1) for p in ("weight", "bias")]
    assert not [n for n in names if n.startswith("iphi.fc_no_code.")]
    assert set(names) == {k for k in init if not k.startswith("iphi.fc_no_code.")}
    assert tr.engine.n_params == sum(v.numel() for k, v in init.items() if not k.startswith("iphi.fc_no_code."))

    val = routine.validation_step(dev(batches[0]))
    assert abs(float(val) - ref_losses[0]) < LOSS_TOL
    for step in range(3):
        loss = routine.training_step(dev(batches[step]), step)
        print(f"step {step}: loss {float(loss):.7f}, oracle {ref_losses[step]:.7f}")
        assert abs(float(loss) - ref_losses[step]) < LOSS_TOL
        assert tr.current_lr() == 1e-3                    # StepLR is per epoch: steps alone do not move it
    got = {k: v.detach().cpu() for k, v in routine.named_parameters()}
    worst = ("", 0.0)
    for k, v in got.items():
        if k.startswith("iphi.fc_no_code."):
            assert torch.equal(v, init[k]), k                  # never written: not even weight decay
            continue
        e = rel_l2(v.numpy(), ref_final[k])
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= PARAM_TOL, (k, e)
        assert not torch.equal(v, init[k]), k
    print(f"worst parameter after three steps: {worst[0]} {worst[1]:.2e}")

    # StepLR(step_size 2, gamma 0.5) through the epoch counter
    for epoch in range(1, 6):
        routine.on_train_epoch_end()
        assert routine.current_epoch == epoch
        assert tr.current_lr() == 1e-3 * 0.5 ** (epoch // 2)
    routine.current_epoch = 0

    # checkpoint round trip: a fresh routine resumed from the file takes the same fourth step
    path = str(tmp_path / "last.ckpt")
    routine.save_checkpoint(path, epoch=0)
    loss4 = float(routine.training_step(dev(batches[3]), 3))
    after4 = {k: v.detach().cpu().clone() for k, v in routine.named_parameters()}
    fresh = _routine(99)
    fresh.to(host_device)
    info = fresh.resume_from_checkpoint(path)
    assert info["global_step"] == 3 and fresh.trainer().step_count == 3 and fresh.trainer().opt_step == 3
    assert float(fresh.training_step(dev(batches[3]), 3)) == loss4
    for k, v in fresh.named_parameters():
        assert torch.equal(v.detach().cpu(), after4[k]), k


def test_the_ffno_model_keeps_adamw_and_the_cosine_schedule():
    from fourierflow_amd.modules import FNOFactorizedPointCloud2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    from fourierflow_amd.routines.point_cloud import _TrainedParameters
    routine = PointCloudExperiment(FNOFactorizedPointCloud2D(M1, M2, W, 2, 1, n_layers=2, s1=S1, s2=S2), IPhi(16), 10)
    assert routine.optimizer_type == "adamw" and routine._step_lr is False
    assert routine._sch_kw == dict(num_warmup_steps=500, num_training_steps=10000, num_cycles=0.5)
    names = [n for n, _ in _TrainedParameters(routine).engine_parameters()]
    assert not [n for n in names if n.startswith("model.ws.") or n.startswith("iphi.fc_no_code.")]
    assert "model.bs.0.weight" in names and "iphi.fc_code.weight" in names


def test_unknown_optimizer_type_is_refused():
    import pytest
    from fourierflow_amd.modules import FNOPointCloud2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    with pytest.raises(NotImplementedError):
        PointCloudExperiment(FNOPointCloud2D(M1, M2, W, 2, 1, n_layers=1, s1=S1, s2=S2), IPhi(16), 10, optimizer_type="sgd")
