"""The 12 shipped geo-FNO elasticity configs (experiments/elasticity/geo-fno*/*/config.yaml, texts in
tests/golden/reference_configs.npz) build PointCloudExperiment + FNOPointCloud2D + IPhi with the one override
``routine.model._target_=fourierflow_amd.modules.FNOPointCloud2D``; model and IPhi kwargs, Adam and StepLR arrive as written.
Without the override each still fails naming FNOPointCloud2D (the name mapping is left out on purpose: DESIGN.md section 7)."""
import os

import numpy as np
import pytest
import yaml

OVERRIDE = "routine.model._target_=fourierflow_amd.modules.FNOPointCloud2D"


def _configs():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs.npz"))
    return dict(zip(z["paths"].tolist(), z["texts"].tolist()))


GEO = sorted(p for p in _configs() if p.startswith(("elasticity/geo-fno/", "elasticity/geo-fno-big/")) and p.endswith("/config.yaml"))


def test_the_fixture_holds_the_twelve_configs():
    assert len(GEO) == 12
    assert {p.split("/")[2] for p in GEO} == {f"{n}_layers" for n in (4, 8, 12, 16, 20, 24)}


@pytest.mark.parametrize("rel", GEO)
def test_shipped_geofno_config_builds_with_the_override(rel, tmp_path):
    from fourierflow_amd.config import build_routine, load_config
    from fourierflow_amd.modules import FNOPointCloud2D, IPhi
    from fourierflow_amd.routines import PointCloudExperiment
    text = _configs()[rel]
    path = tmp_path / "config.yaml"
    path.write_text(text)
    routine = build_routine(load_config(str(path), [OVERRIDE]))
    raw = yaml.safe_load(text)["routine"]
    assert raw["model"]["_target_"] == "fourierflow.modules.FNOPointCloud2D"
    assert type(routine) is PointCloudExperiment and routine.N == raw["N"]
    assert type(routine.model) is FNOPointCloud2D and type(routine.iphi) is IPhi
    for k, v in raw["model"].items():
        if not k.startswith("_"):
            assert getattr(routine.model, k) == v, k
    n = raw["model"]["n_layers"]
    assert n == int(rel.split("/")[2].split("_")[0]) == routine.model.n_layers       # untouched: 4_layers trains 4 layers
    assert len(routine.model.convs) == n + 1 and len(routine.model.bs) == n + 1 and len(routine.model.ws) == n - 1
    assert routine.iphi.width == raw["iphi"]["width"]
    opt = {k: v for k, v in raw["optimizer"].items() if not k.startswith("_")}
    sch = {k: v for k, v in raw["scheduler"]["scheduler"].items() if not k.startswith("_")}
    assert opt == dict(lr=0.001, weight_decay=0.0001) and sch == dict(step_size=50, gamma=0.5)
    assert routine.optimizer_type == "adam" and routine._step_lr
    assert {k: routine._opt_kw[k] for k in opt} == opt
    assert {k: routine._sch_kw[k] for k in sch} == sch


@pytest.mark.parametrize("rel", GEO)
def test_without_the_override_the_config_is_refused_by_name(rel, tmp_path):
    from fourierflow_amd.config import build_routine, load_config
    path = tmp_path / "config.yaml"
    path.write_text(_configs()[rel])
    with pytest.raises(NotImplementedError, match="FNOPointCloud2D"):
        build_routine(load_config(str(path)))


def test_adam_stays_refused_for_the_ffno_point_cloud_model(tmp_path):
    from fourierflow_amd.config import build_routine, load_config
    path = tmp_path / "config.yaml"
    path.write_text(_configs()[GEO[0]])
    with pytest.raises(NotImplementedError, match="AdamW"):
        build_routine(load_config(str(path), ["routine.model._target_=fourierflow.modules.FNOFactorizedPointCloud2D"]))
