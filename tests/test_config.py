"""an experiment config in the reference's schema (torus_li/markov style: Hydra `_target_` nodes,
`${get_method:...}` resolvers, functools.partial optimiser/scheduler factories) builds the HIP-backed routine."""
import os

import numpy as np
import pytest
import torch

from backend_util import host_device  # noqa: F401

CONFIG = """
wandb:
  project: torus_li
  group: markov/test
builder:
  _target_: fourierflow.builders.NSMarkovBuilder
  data_path: ${oc.env:DATA_ROOT}/zongyi/NavierStokes_V1e-5_N1200_T20.mat
  batch_size: 2
routine:
  _target_: fourierflow.routines.Grid2DMarkovExperiment
  conv:
    _target_: fourierflow.modules.FNOFactorized2DBlock
    modes: 4
    width: 64
    n_layers: 2
    input_dim: 3
    share_weight: true
    factor: 4
    ff_weight_norm: true
    gain: 0.1
    dropout: 0.0
    in_dropout: 0.0
  n_steps: 10
  max_accumulations: 1000
  noise_std: 0.01
  optimizer:
    _target_: functools.partial
    _args_: ["${get_method: torch.optim.AdamW}"]
    lr: 0.0025
    weight_decay: 0.0001
  scheduler:
    scheduler:
      _target_: functools.partial
      _args_: ["${get_method: fourierflow.schedulers.CosineWithWarmupScheduler}"]
      num_warmup_steps: 500
      num_training_steps: 100000
      num_cycles: 0.5
    name: learning_rate
trainer:
  accelerator: gpu
  devices: 1
  precision: 32
callbacks:
  - _target_: pytorch_lightning.callbacks.LearningRateMonitor
    logging_interval: step
"""


def test_reference_style_config_builds_and_trains(tmp_path, host_device):
    from fourierflow_amd.config import build_routine, load_config
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    path = tmp_path / "config.yaml"
    path.write_text(CONFIG)
    cfg = load_config(str(path), ["routine.conv.n_layers=3", "routine.noise_std=0.0", "routine.conv.modes=4"])
    assert cfg["routine"]["conv"]["n_layers"] == 3
    routine = build_routine(cfg).to(host_device)
    assert isinstance(routine, Grid2DMarkovExperiment) and isinstance(routine.conv, FNOFactorized2DBlock)
    assert routine.conv.n_layers == 3 and routine.noise_std == 0.0 and routine.n_steps == 10
    tr = routine.trainer()
    assert (tr.lr, tr.wd, tr.sched) == (0.0025, 0.0001, (500, 100000, 0.5))
    B, G = 2, 8
    mk = lambda: dict(x=torch.randn(B, G, G, 1, device=host_device), y=torch.randn(B, G, G, 1, device=host_device))  # noqa: E731
    assert routine.training_step(mk(), epoch=0) is None
    losses = [routine.training_step(mk(), epoch=1).item() for _ in range(2)]
    assert all(l == l and l > 0 for l in losses) and tr.step_count == 2


def test_unknown_reference_targets_fail_loudly(tmp_path):
    from fourierflow_amd.config import instantiate
    from fourierflow_amd.modules import FNOFactorized2DBlock
    from fourierflow_amd.routines import Grid2DMarkovExperiment
    conv = FNOFactorized2DBlock(modes=4, width=32, n_layers=1, input_dim=3)
    Grid2DMarkovExperiment(conv, clip_val=None, automatic_optimization=False, accumulate_grad_batches=1)   # reference defaults
    with pytest.raises(NotImplementedError, match="clip_val"):
        Grid2DMarkovExperiment(conv, clip_val=0.1)
    with pytest.raises(NotImplementedError, match="accumulate_grad_batches"):
        Grid2DMarkovExperiment(conv, accumulate_grad_batches=4)
    with pytest.raises(NotImplementedError):
        instantiate({"_target_": "fourierflow.modules.FNOPointCloud2D", "modes1": 12})
    with pytest.raises(ValueError):
        instantiate("${nope: 1}")
    assert instantiate("${eval: 2 * 3}") == 6


REFERENCE_CONFIGS = [
    ("torus_li/markov/24_layers", "Grid2DMarkovExperiment", "conv", "FNOFactorized2DBlock"),
    ("torus_li/markov/4_layers", "Grid2DMarkovExperiment", "conv", "FNOFactorized2DBlock"),
    ("plasticity/ffno/12_layers", "StructuredMeshExperiment", "model", "FNOFactorizedMesh3D"),
    ("airfoil/ffno/24_layers", "StructuredMeshExperiment", "model", "FNOFactorizedMesh2D"),
    ("pipe/ffno/8_layers", "StructuredMeshExperiment", "model", "FNOFactorizedMesh2D"),
    ("torus_kochkov/ffno/ablation/fno++/128", "Grid2DMarkovExperiment", "conv", "FNOPlus2DBlock"),
    ("torus_kochkov/ffno/grid_sizes/256", "Grid2DMarkovExperiment", "conv", "FNOFactorized2DBlock"),
    ("torus_li/zongyi/4_layers", "Grid2DRolloutExperiment", "conv", "FNOZongyi2DBlock"),       # BASELINE config 0
    ("pipe/geo-fno/8_layers", "StructuredMeshExperiment", "model", "FNOMesh2D"),               # geo-FNO baseline, Adam + StepLR
    ("plasticity/geo-fno/4_layers", "StructuredMeshExperiment", "model", "FNOMesh3D"),
    ("plasticity/fcno/12_layers", "StructuredMeshExperiment", "model", "CNOFactorizedMesh3D"),   # DCT operators
]


def shipped_configs():
    """{path under the reference's experiments/: YAML text} of all its config.yaml files, stored as test data
    (tests/golden/reference_configs.npz, written by tools/make_config_fixture.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs.npz"))
    return dict(zip(z["paths"].tolist(), z["texts"].tolist()))


@pytest.mark.parametrize("rel,routine_cls,attr,model_cls", REFERENCE_CONFIGS)
def test_shipped_experiment_configs_build_unchanged(rel, routine_cls, attr, model_cls, tmp_path):
    """The reference's own experiments/**/config.yaml files (stored verbatim under tests/golden/) instantiate the
    native routine + operator without edits: same `_target_`s, kwargs, optimiser and schedule."""
    text = shipped_configs()[rel + "/config.yaml"]
    path = tmp_path / "config.yaml"
    path.write_text(text)
    import yaml
    from fourierflow_amd.config import build_routine, load_config
    # the non-factorized configs carry ~0.5 GB of [C, C, K, K, 2] weights per 24 layers: two layers are enough to check
    # that every constructor argument of the file arrives
    shrink = [f"routine.{attr}.n_layers=2"] if model_cls in ("FNOPlus2DBlock", "FNOMesh3D") else []
    cfg = load_config(str(path), shrink)
    routine = build_routine(cfg)
    assert type(routine).__name__ == routine_cls
    model = getattr(routine, attr)
    assert type(model).__name__ == model_cls
    raw = yaml.safe_load(text)["routine"]
    for k, v in raw[attr].items():
        if not k.startswith("_") and isinstance(v, (int, float, bool)) and hasattr(model, k) and not (shrink and k == "n_layers"):
            assert getattr(model, k) == v, k
    opt = {k: v for k, v in raw["optimizer"].items() if not k.startswith("_")}
    sch = {k: v for k, v in raw["scheduler"]["scheduler"].items() if not k.startswith("_")}
    assert {k: routine._opt_kw[k] for k in opt} == opt
    assert {k: routine._sch_kw[k] for k in sch} == sch


def test_every_shipped_ffno_config_builds(tmp_path):
    """Sweep of the reference's 256 experiment configs (stored under tests/golden/): everything built on the F-FNO operators
    of SURVEY 8 instantiates unchanged; the rest fails LOUDLY with a reason from a short, explicit list."""
    configs = shipped_configs()
    assert len(configs) == 256, len(configs)
    from fourierflow_amd.config import build_routine, load_config
    known = ("FNOZongyi2DBlock", "width > 32", "FNOMesh2D", "FNOMesh3D", "PointCloud", "CNOFactorized", "IPhi",
             "only torch.optim.AdamW", "only CosineWithWarmupScheduler", "optax", "use_fourier_position",
             "MeshGraphNet", "LearnedInterpolator", "Grid2DRolloutExperiment")
    built, unexpected = 0, []
    for rel, text in configs.items():
        p = tmp_path / "config.yaml"
        p.write_text(text)
        try:
            cfg = load_config(str(p))
            node = cfg.get("routine", {})
            for key in ("conv", "model"):                 # one layer is enough to exercise every constructor argument
                if isinstance(node.get(key), dict) and "n_layers" in node[key]:
                    node[key]["n_layers"] = 1
            build_routine(cfg)
            built += 1
        except (NotImplementedError, ModuleNotFoundError) as e:
            if not any(k in str(e) for k in known):
                unexpected.append((rel, repr(e)))
        except Exception as e:  # noqa: BLE001 - anything else is a loader bug
            unexpected.append((rel, repr(e)))
    assert not unexpected, unexpected[:5]
    assert built >= 218, built
