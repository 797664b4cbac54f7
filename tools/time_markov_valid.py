#!/usr/bin/env python3
"""Time of one validation batch of the Markov routine (batch 19, 64 x 64, 24 layers, 10 steps) on the GPU: validation_step
(ffno_markov_traj_step / ffno_markov_traj_metrics) against rollout() + the same metrics in eager torch.  Median of 5 rounds
of 20 calls, the two sides alternating; one JSON line.  DESIGN.md section 4, "Trajectory validation of the Markov routine".
Run from the repository root:  python tools/time_markov_valid.py"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fourierflow_amd.modules import FNOFactorized2DBlock
from fourierflow_amd.routines import Grid2DMarkovExperiment

KW = dict(modes=16, width=64, n_layers=24, input_dim=3, share_weight=True, factor=4, ff_weight_norm=True, gain=0.1)
B, G, T, N = 19, 64, 11, 10
dev = "cuda:0"
torch.manual_seed(0)
exp = Grid2DMarkovExperiment(FNOFactorized2DBlock(**KW), n_steps=N).to(dev)
data = torch.randn(B, G, G, T, device=dev)
for _ in range(2):
    exp.training_step(dict(x=torch.randn(B, G, G, 1, device=dev), y=torch.randn(B, G, G, 1, device=dev)), epoch=0)
exp.eval()
batch = dict(data=data)


def new():
    v = exp.validation_step(batch)
    return float(v["valid_loss"]), v["valid_time_until"]


def old():
    with torch.no_grad():
        preds = exp.rollout(data[..., T - N - 1].unsqueeze(-1).contiguous(), N)
        yy = data[..., -N:]
        nrm = lambda a, d: torch.norm(a, dim=d)      # noqa: E731
        step = (nrm((preds - yy).reshape(B, -1, N), 1) / nrm(yy.reshape(B, -1, N), 1)).mean(0)
        loss = step.sum() / N
        full = (nrm((preds - yy).reshape(B, -1), 1) / nrm(yy.reshape(B, -1), 1)).mean()
        p = ((preds / torch.norm(preds, dim=[1, 2], keepdim=True)) * (yy / torch.norm(yy, dim=[1, 2], keepdim=True)))
        p = p.sum(dim=[1, 2]).mean(dim=0)
        below = (p < 0.95).nonzero()
        t_until = float(below[0, 0]) if len(below) else float(N)
        nan = bool(torch.isnan(loss)) or bool(torch.isnan(full))      # the NaN rule's host reads (:397-400)
        return (9999.9 if nan else float(full)), t_until


def timed(fn, reps=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps, r


for fn in (new, old):
    timed(fn, 3)
rounds = {"new": [], "old": []}
for _ in range(5):
    t, rn = timed(new)
    rounds["new"].append(t)
    t, ro = timed(old)
    rounds["old"].append(t)
print(json.dumps(dict(new_ms=statistics.median(rounds["new"]), old_ms=statistics.median(rounds["old"]), rounds=rounds,
                      new=rn, old=ro)))
