"""PointCloudExperiment with the fully factorised point-cloud F-FNO (FNOFullyFactorizedMesh2D + IPhi, AdamW under the cosine
schedule, the routine unchanged): three training steps follow float64 autograd through the restatement of
tests/pointcloud_fullyfact_oracle.py + torch.optim.AdamW + the cosine LambdaLR (loss within 2e-5 x max(1, loss) per step,
parameters <= 5e-4 rel-L2 afterwards: the bands of tests/test_pointcloud_routine.py, whose losses are of order 1; this model's
Fourier weights are Xavier-initialised, its first losses are near 40, where one fp32 ulp of the loss itself is 3.8e-6, so the
loss band is stated relative to the oracle's loss); the registered-but-unused parameters (ws.*, the last layer's
backcast_ff, iphi.fc_no_code.*) stay out of the flat buffer and are bit-unchanged; validation is the no-grad loss; a checkpoint
resumes to the same next step."""
import numpy as np
import torch

import pointcloud_fullyfact_oracle as pfo
import pointcloud_model_oracle as pmo
from backend_util import host_device, rel_l2  # noqa: F401  (host_device is a fixture)

B, W, M1, M2, S, N, L = 2, 32, 4, 3, 10, 37, 3
OPT = dict(lr=1e-3, weight_decay=1e-4)
SCH = dict(num_warmup_steps=2, num_training_steps=10, num_cycles=0.5)
LOSS_TOL, PARAM_TOL = 2e-5, 5e-4
UNUSED = ("model.ws.", f"model.convs.{L}.backcast_ff.", "iphi.fc_no_code.")


def _routine(seed):
    from fourierflow_amd.modules import FNOFullyFactorizedMesh2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    torch.manual_seed(seed)
    model = FNOFullyFactorizedMesh2D(M1, M2, W, 2, 1, n_layers=L, s1=S, s2=S)
    return PointCloudExperiment(model, IPhi(16), 10, optimizer=dict(OPT), scheduler=dict(SCH))


def _batches(n_steps, seed):
    rng = np.random.default_rng(seed)
    return [dict(xy=rng.uniform(0.05, 0.95, (B, N, 2)).astype(np.float32), rr=rng.standard_normal((B, 42)).astype(np.float32),
                 sigma=rng.standard_normal((B, N, 1)).astype(np.float32)) for _ in range(n_steps)]


def _oracle_training(routine, batches):
    """float64 autograd through the restatement + torch.optim.AdamW + the cosine LambdaLR: losses, final unique parameters.
    Parameters without a gradient are skipped by torch.optim.AdamW, weight decay included."""
    from oracle import ffno_oracle as orc
    sd, uniq = pmo.model_state_dict(routine.model.state_dict(), torch.float64)
    isd, iuniq = pmo.model_state_dict(routine.iphi.state_dict(), torch.float64)
    opt = torch.optim.AdamW(list(uniq.values()) + list(iuniq.values()), **OPT)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda s: orc.cosine_warmup_factor(s, SCH["num_warmup_steps"], SCH["num_training_steps"], SCH["num_cycles"]))
    losses = []
    for b in batches:
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in b.items()}
        out = pfo.model(sd, t["xy"], t["rr"], iphi_sd=isd, iphi_width=routine.iphi.width, modes1=M1, modes2=M2, width=W,
                        n_layers=L, s=S)
        loss = pmo.rel_l2_loss(out, t["sigma"])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss.detach()))
    final = {"model." + k: v for k, v in uniq.items()}
    final.update({"iphi." + k: v for k, v in iuniq.items()})
    return losses, {k: v.detach().numpy() for k, v in final.items()}


def test_three_training_steps_follow_the_oracle(host_device, tmp_path):
    routine = _routine(50)
    batches = _batches(4, 51)
    ref_losses, ref_final = _oracle_training(routine, batches[:3])
    init = {k: v.detach().clone() for k, v in routine.named_parameters()}
    routine.to(host_device)
    dev = lambda b: {k: torch.tensor(v, device=host_device) for k, v in b.items()}      # noqa: E731

    with torch.no_grad():
        plain = pmo.rel_l2_loss(routine(dev(batches[0])), dev(batches[0])["sigma"])
    val = routine.validation_step(dev(batches[0]))
    assert abs(float(val) - float(plain)) < 1e-6 * max(1.0, abs(float(plain)))
    assert abs(float(val) - ref_losses[0]) < LOSS_TOL * max(1.0, abs(ref_losses[0]))

    tr = routine.trainer()
    assert tr.decoupled is True
    names = list(tr.engine.param_names)
    assert not [n for n in names if n.startswith(UNUSED)]
    assert set(names) == {k for k in init if not k.startswith(UNUSED)} and len(names) == len(set(names))
    assert len([k for k in init if k.startswith(UNUSED)]) == 2 * (L - 1) + 6 + 2
    for step in range(3):
        loss = routine.training_step(dev(batches[step]), step)
        print(f"step {step}: loss {float(loss):.6f}, oracle {ref_losses[step]:.6f}")
        assert abs(float(loss) - ref_losses[step]) < LOSS_TOL * max(1.0, abs(ref_losses[step]))
    got = {k: v.detach().cpu() for k, v in routine.named_parameters()}
    worst = ("", 0.0)
    for k, v in got.items():
        if k.startswith(UNUSED):
            assert torch.equal(v, init[k]), k                  # never written: not even weight decay
            assert np.array_equal(ref_final[k], init[k].numpy().astype(np.float64)), k      # nor by torch.optim.AdamW
            continue
        e = rel_l2(v.numpy(), ref_final[k])
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= PARAM_TOL, (k, e)
        assert not torch.equal(v, init[k]), k
    print(f"worst parameter after three steps: {worst[0]} {worst[1]:.2e}")

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
