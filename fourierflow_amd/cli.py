"""`python -m fourierflow_amd {train,test,predict} CONFIG.yaml [overrides...]`, `python -m fourierflow_amd rollout CONFIG.yaml
--init IC.npz` (the trained Markov model as a simulator, see `rollout` below) and `python -m fourierflow_amd generate
navier-stokes PATH` / `generate kolmogorov X.yaml` (the data the 2-D Navier-Stokes and the Kolmogorov-flow configs train on, see
`navier_stokes` and `kolmogorov` below) -- the command surface of the reference
(`fourierflow train | test | predict | infer`, reference commands/train.py:27-148, commands/test.py:24-90,
commands/predict.py:24-110, commands/infer.py) for the routines built here, with the same positional arguments and flag names
(``--force --resume --checkpoint-id --trial --debug --no-logging --map-location``) and the same on-disk layout:

    <config_dir>/checkpoints/trial-<trial>-<id>/epoch=<e>-step=<s>-valid_loss=<v>.ckpt   (best, what `test` / `predict` load)
    <config_dir>/checkpoints/trial-<trial>-<id>/last.ckpt                                 (what `--resume` continues from)
    (KolmogorovBuilder configs under `--builder`: the best file is chosen and named by the config's CustomModelCheckpoint entry,
     epoch=<e>-step=<s>-valid_time_until=<v>.ckpt for the torus_kochkov configs)

What is NOT here is the reference's control plane: Hydra (the loader of fourierflow_amd/config.py resolves the same
interpolations), Lightning (the routines run their own fused step), wandb (one JSON line per logged step on stdout)
and most dataset builders.  Without ``--builder``, batches come from ``--data FILE.npz`` (arrays named like
the builder's batches: ``x``/``y`` [, ``f``, ``mu``] for the Markov and mesh routines, ``data`` for the rollout routine;
for the Markov routine a file with ``data`` [n, M, N, T] [, ``times``, ``f``, ``mu``, ``corr_data``] is a TRAJECTORY file, what
its validation / test loaders deliver: `test --data` and `train --valid-data` run the autoregressive metrics on it, and
`train --data` with any of ``--pair-mode --pair-stride --epochs --no-shuffle --drop-last`` draws shuffled one-step pairs from it
on the device (builders/markov_data.py; without one of these options a trajectory training file is refused);
``xy``/``rr``/``sigma`` for the point-cloud routine; first axis = samples) or, without it, are synthetic N(0,1) fields of the
configured geometry (point clouds: ``xy`` uniform in [0, 1)^2, 972 points unless ``--size``, ``rr`` [B, 42], ``sigma`` [B, n, 1]).

``train CONFIG --builder`` and ``test CONFIG --builder`` run the routines the way the reference does: on the dataset files of the
config's ``builder`` section (StructuredMesh2DBuilder, PlasticityBuilder, ElasticityBuilder: builders/mesh_data.py; NSMarkovBuilder,
NSZongyiBuilder: builders/ns_data.py; NSContextualBuilder: builders/ns_contextual.py; KolmogorovBuilder: builders/kolmogorov.py),
split by ``train_size`` / ``valid_size`` / ``test_size`` (NSContextualBuilder: by its train / valid / test files; KolmogorovBuilder: by
the files of its three dataset nodes, each ``P.nc`` read from ``P.npz`` beside it), in shuffled epochs drawn on the
device, with the validation split evaluated after every epoch and the best checkpoint kept.  For the Markov routine epoch 0 is
the reference's statistics epoch: one whole pass that only accumulates the normaliser.  ``predict CONFIG --builder`` runs on the
builder's ``inference_data()`` and reports the reference's ``inference_time``; NSContextualBuilder has none, in the reference
either, and is refused there.  With KolmogorovBuilder the routine reduces its predictions to the grid of ``corr_data`` on the device
(``downsample_corr``), ``valid_corr`` / ``valid_reduced_time_until`` are the reduced ones, the checkpoint is selected by the config's
``CustomModelCheckpoint`` entry (``valid_time_until``, max) and `test --builder` also prints ``test_reduced_time_until``.  Its
multi-resolution configs (torus_kochkov/ffno/multi_resolution) take the one override
``builder.train_dataset._target_=fourierflow_amd.builders.KolmogorovMultiResolutionDataset``: training batches then alternate between
the grid sizes of ``paths`` in the order the reference's loader workers serve them (builders/markov_data.py), the statistics epoch
covers both sizes, and validation, test and predict run at the validation files' own size.

``test CONFIG [--builder | --data TRAJ.npz] [--pred-path P]``: a Markov routine with a ``pred_path`` (the
torus_kochkov/ffno/predictions configs set ``routine.pred_path``; ``--pred-path`` overrides it) exports every test prediction on its
``pred_size`` grid -- vorticity, vx, vy and their energy spectrum (diagnostics.py) -- and the command writes ONE file for all test
batches, the ``.npz`` sibling of the path, reporting ``pred_path`` (the file written) and ``pred_samples``.
"""
from __future__ import annotations

import json
import math
import time
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch
from typer import Argument, BadParameter, Option, Typer

from .builders.file_batches import Batches, holds_trajectories, initial_conditions, trajectory_batches
from .builders.synthetic import Force
from .config import build_routine, load_config
from .routines import routine_kind

app = Typer(add_completion=False, help=__doc__)
_LAST: Dict[str, object] = {}


def _last_routine():
    """The routine object the last `train` command of this process built (for callers that drive the CLI in-process)."""
    return _LAST.get("routine")


# ------------------------------------------------------------------------------------------------------------------
def _device(device: Optional[str]) -> torch.device:
    return torch.device(device or "cuda:0")


def _init_distributed(device: Optional[str]):
    """(rank, world, device).  Started as one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m
    fourierflow_amd train ...`: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment) the command joins the job --
    the counterpart of the reference handing Lightning a DDPPlugin (commands/train.py:83-84): weights are broadcast from
    rank 0, every rank draws its own shard of each global batch, the flat gradient buffer is all-reduced once per step
    (FFNOTrainer) and the normaliser statistics are global (Normalizer.sync_across_ranks).  RCCL on GPUs, gloo on CPU tensors."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1 or "RANK" not in os.environ:
        return 0, 1, _device(device)
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device(device) if device else torch.device("cuda", local)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    if not torch.distributed.is_initialized():
        torch.distributed.init_process_group("nccl" if dev.type == "cuda" else "gloo", rank=rank, world_size=world)
    return rank, world, dev


def _now(dev: torch.device) -> float:
    """The wall clock once the work queued on the device is done: the two ends of every timed loop."""
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return time.perf_counter()


def _open_run(run):
    """The trial directory of a training run and where it starts: checkpoints and the log lines are rank 0's (every rank holds
    the same weights and the same global normaliser statistics), so `run.out_dir` is None on the others and without logging;
    --force deletes the old checkpoints (delete_old_results, commands/train.py:58); --resume continues from last.ckpt, which
    every rank reads (`run.last`), and `run.start` is its epoch and global step."""
    trial_dir = None if run.no_logging else _trial_dir(run.config_path.parent, run.trial, run.checkpoint_id, create=run.rank == 0)
    run.out_dir = trial_dir if run.rank == 0 else None
    if run.out_dir is not None and run.force and not run.resume:
        for old in run.out_dir.glob("*.ckpt"):
            old.unlink()
    run.start, run.last = dict(epoch=0, global_step=0), None
    if run.resume:
        if trial_dir is None or not (trial_dir / "last.ckpt").exists():
            raise FileNotFoundError("--resume needs checkpoints/trial-<trial>-*/last.ckpt (commands/train.py:74-80)")
        run.last = trial_dir / "last.ckpt"
        run.start = run.routine.resume_from_checkpoint(str(run.last))
    return run.out_dir, run.start


def _load_trained(config_path: Path, overrides, trial: int, map_location, device, accept=None):
    """(cfg, routine, kind, ckpt): the routine of CONFIG with the weights of the trial's best checkpoint (or the
    `checkpoint_path=...` override), on the device and under eval() -- trainer.test / predict run so: no statistics accumulation
    (commands/test.py, normalizer.py:48).  `accept(routine, kind)`, where given, sees the routine before a checkpoint is looked
    for: a command's own refusals come first."""
    cfg = load_config(str(config_path), overrides or [])
    dev = _device(device)
    routine = build_routine(cfg).to(dev)
    kind = routine_kind(routine)
    if accept is not None:
        accept(routine, kind)
    ckpt = _best_checkpoint(config_path.parent, trial, cfg.get("checkpoint_path"))
    routine.load_lightning_model_state(str(ckpt), map_location)
    routine.to(dev)
    routine.eval()
    return cfg, routine, kind, ckpt


# the classes `--builder` runs and the routine each one feeds
BUILDERS = {"StructuredMesh2DBuilder": "mesh", "PlasticityBuilder": "mesh", "ElasticityBuilder": "pointcloud",
            "NSMarkovBuilder": "markov", "NSZongyiBuilder": "rollout", "NSContextualBuilder": "markov",
            "KolmogorovBuilder": "markov"}
_ROUTINES = {"mesh": "StructuredMeshExperiment", "pointcloud": "PointCloudExperiment", "markov": "Grid2DMarkovExperiment",
             "rollout": "Grid2DRolloutExperiment"}


def _instantiate_builder(cfg, kind: str, batch_size: Optional[int], routine=None):
    """The config's `builder` section as one of builders/mesh_data.py / ns_data.py / ns_contextual.py / kolmogorov.py (`${oc.env:DATA_ROOT}` resolved like everywhere
    else).  A section that names another builder than the routine's, none at all, or lacks an argument its class requires is
    refused before anything is read."""
    import inspect

    from .config import TARGET_MAP, import_string, instantiate
    node = dict(cfg.get("builder") or {})
    target = str(node.get("_target_", ""))
    name = target.rpartition(".")[2]
    runs = "; ".join(f"{_ROUTINES[k]} on {' / '.join(b for b, kk in BUILDERS.items() if kk == k)}" for k in _ROUTINES)
    if BUILDERS.get(name) != kind:
        raise ValueError(f"--builder runs {runs}; this config pairs a {kind} routine with builder {name or '(none)'!r}")
    cls = import_string(TARGET_MAP.get(target, target))
    missing = [p.name for p in inspect.signature(cls.__init__).parameters.values()
               if p.name != "self" and p.default is p.empty and p.kind is p.POSITIONAL_OR_KEYWORD and p.name not in node]
    if missing:
        raise ValueError(f"the builder section of this config lacks {', '.join(missing)}, which {name} requires (--builder runs "
                         f"{runs})")
    if batch_size:
        node["batch_size"] = batch_size
    bld = instantiate(node)
    if routine is not None and hasattr(bld, "append_force"):      # f / mu go along when the routine appends them
        bld.append_force, bld.append_mu = bool(routine.append_force), bool(routine.append_mu)
    if name == "KolmogorovBuilder" and routine is not None:      # its corr_data lives on a coarser grid than the model (32 x 32)
        routine.downsample_corr = True
    if kind == "rollout" and routine is not None and \
            (bld.n_steps != routine.n_steps or bld.append_pos != bool(routine.append_pos)):
        raise ValueError(f"builder n_steps = {bld.n_steps}, append_pos = {bld.append_pos} but the routine rolls out n_steps = "
                         f"{routine.n_steps} with append_pos = {bool(routine.append_pos)}: the batches would not fit")
    return bld


def _split_loss(routine, data, step: str = "validation_step", keys=None, each=None) -> Dict[str, float]:
    """The sample-weighted mean, over every batch of `data` (short last batch included), of every key that `step` logs -- what
    Lightning logs for the epoch -- under eval().  A routine whose step returns the loss alone gives {'valid_loss': ...}.  Tensor
    values are accumulated on the device and read once at the end; `keys` picks from a step that returns more (per-step tables);
    `each`, where given, sees every batch's whole output."""
    was_training = routine.training
    routine.eval()
    try:
        with torch.no_grad():
            totals, n = {}, 0
            for batch in data.epoch():
                B = len(next(iter(batch.values())))
                out = getattr(routine, step)(batch)
                if not isinstance(out, dict):
                    out = {"valid_loss": out}
                if each is not None:
                    each(out)
                for k in (keys or out):
                    v = out[k]
                    part = (v.reshape(()).double() if torch.is_tensor(v) else float(v)) * B
                    totals[k] = part if k not in totals else totals[k] + part
                n += B
            return {k: float(v) / n for k, v in totals.items()}
    finally:
        routine.train(was_training)


class _PredictionParts:
    """The exported arrays of every test batch of a Markov routine with a pred_path, on the host, and the one file they make."""

    def __init__(self, routine):
        self.routine, self.parts, self.times = routine, [], None

    def __call__(self, out):
        from .diagnostics import PRED_KEYS
        self.parts.append({k: out[k].cpu() for k in PRED_KEYS})
        if self.times is None and "test_times" in out:
            self.times = out["test_times"].cpu()

    def write(self) -> Dict[str, object]:
        path = self.routine.write_predictions(None, self.parts, self.times)
        return dict(pred_path=path, pred_samples=sum(p["pred_vorticity"].shape[1] for p in self.parts))


TEST_KEYS = {"markov": ("test_loss", "test_loss_avg", "test_time_until", "test_corr"),
             "rollout": ("test_loss", "test_loss_avg", "test_time_until")}


def _checkpoint_rule(cfg, bld):
    """(monitor, mode, file name template) of the best checkpoint.  Every builder but KolmogorovBuilder: valid_loss / min and the
    name epoch=<e>-step=<s>-valid_loss=<v>.ckpt (template None).  KolmogorovBuilder: the config's CustomModelCheckpoint entry
    (torus_kochkov: monitor valid_time_until, mode max, filename "{epoch}-{step}-{valid_time_until:.3f}"), the name written the way
    Lightning writes it: every `{key` of the template becomes `key={key`."""
    if type(bld).__name__ != "KolmogorovBuilder":
        return "valid_loss", "min", None
    entry = next((c for c in (cfg.get("callbacks") or []) if isinstance(c, dict) and
                  str(c.get("_target_", "")).endswith("CustomModelCheckpoint")), {})
    monitor, mode = str(entry.get("monitor", "valid_loss")), str(entry.get("mode", "min"))
    if mode not in ("min", "max"):
        raise ValueError(f"CustomModelCheckpoint.mode is min or max, got {mode!r}")
    return monitor, mode, str(entry.get("filename") or "{epoch}-{step}-{%s:.5f}" % monitor)


def _checkpoint_name(template: str, **values) -> str:
    import re
    return re.sub(r"\{([A-Za-z_]\w*)", r"\1={\1", template).format(**values) + ".ckpt"


def _train_from_builder(run, epochs, no_shuffle, drop_last, batch_size):
    """`train --builder`: whole epochs over the builder's training split, validation over its whole validation split after every
    epoch, the best checkpoint kept (CustomModelCheckpoint: monitor valid_loss, mode min, top 1), last.ckpt every epoch.  The
    Markov routine with `should_normalize` spends epoch 0 on the normaliser statistics alone (grid_2d_markov.py:374-390): no
    optimisation step is taken, `global_step` stands still, and the epoch is validated and checkpointed like any other."""
    cfg, routine, kind, dev, rank, world = run.cfg, run.routine, run.kind, run.dev, run.rank, run.world
    bld = _instantiate_builder(cfg, kind, batch_size, routine)
    monitor, mode, template = _checkpoint_rule(cfg, bld)
    worst = math.inf if mode == "min" else -math.inf
    n_epochs = epochs or int((cfg.get("trainer") or {}).get("max_epochs", 0))
    if n_epochs < 1:
        raise ValueError("--builder runs whole epochs: pass --epochs E or set trainer.max_epochs in the config")
    train_set = bld.train_data(dev, seed=7231 + run.trial, rank=rank, world=world, shuffle=not no_shuffle, drop_last=drop_last)
    valid_set = bld.valid_data(dev)      # every rank validates the whole split
    (out_dir, start), best = _open_run(run), worst
    if run.last is not None:
        # the best validation loss so far: last.ckpt carries it, as Lightning's carries its checkpoint callback's state
        saved = torch.load(str(run.last), map_location="cpu", weights_only=False).get("callbacks") or {}
        best = float((saved.get("ModelCheckpoint") or {}).get("best_model_score", worst))
        train_set.skip_epochs(start["epoch"])      # the permutations of the epochs already run
    routine.current_epoch = start["epoch"]
    t0 = _now(dev)
    gs = start["global_step"]
    for epoch in range(start["epoch"], n_epochs):
        loss = None
        for batch in train_set.epoch():
            loss = _train_step(routine, kind, batch, epoch, gs)      # None in the Markov routine's statistics epoch
            gs += loss is not None
        lv, lr = None if loss is None else float(loss.item()), routine.trainer().current_lr()
        if lv is not None and not math.isfinite(lv):
            raise FloatingPointError(f"non-finite training loss at the end of epoch {epoch} (step {gs - 1}): check the data and the "
                                     f"learning rate")
        if hasattr(routine, "on_train_epoch_end"):
            routine.on_train_epoch_end()
        valid = _split_loss(routine, valid_set)
        if monitor not in valid:
            raise KeyError(f"the checkpoint monitor {monitor!r} is not among the validation keys {sorted(valid)}")
        score = valid[monitor]
        vl = valid.pop("valid_loss")
        improved = score < best if mode == "min" else score > best      # strictly better, or the earlier file stays
        if out_dir is not None:
            if improved:
                for old in out_dir.glob("epoch*.ckpt"):
                    old.unlink()
                name = f"epoch={epoch + 1}-step={gs}-valid_loss={vl:.5f}.ckpt" if template is None else \
                    _checkpoint_name(template, epoch=epoch + 1, step=gs, valid_loss=vl, **valid)
                routine.save_checkpoint(str(out_dir / name), epoch=epoch + 1, global_step=gs)
        best = score if improved else best
        if out_dir is not None:
            last = routine.checkpoint_dict(epoch + 1, gs)
            last["callbacks"] = {"ModelCheckpoint": dict(monitor=monitor, best_model_score=best)}
            torch.save(last, str(out_dir / "last.ckpt"))
        if rank == 0:
            print(json.dumps(dict(epoch=epoch + 1, step=gs, train_loss=None if lv is None else round(lv, 6), lr=lr,
                                  valid_loss=round(vl, 6), best=improved, **{k: round(v, 6) for k, v in valid.items()})),
                  flush=True)
    dt = _now(dev) - t0
    steps = gs - start["global_step"]
    if rank == 0:
        print(json.dumps(dict(steps=steps, batch=train_set.batch_size, world_size=world, epochs=n_epochs - start["epoch"],
                              steps_per_s=round(steps / max(dt, 1e-9), 2), resumed_from_step=start["global_step"],
                              **({} if best == worst else {monitor: round(best, 6)}))), flush=True)
    if world > 1:
        torch.distributed.barrier()


def _train_step(routine, kind, batch, epoch, step):
    """One training step of the routine -> its loss (the Markov routine's statistics epoch: None)."""
    if kind == "markov":
        return routine.training_step(batch, epoch=epoch)
    out = routine.training_step(batch, step)
    return out[0] if kind == "rollout" else out


def _valid_loss(routine, kind, batch) -> float:
    """`valid_loss` of the checkpoint file name: the routine's validation metric on one batch."""
    # the reference validates / tests under model.eval(): the Normalizer must NOT accumulate the validation batch into its
    # running statistics (normalizer.py:45-49) -- and they must not leak into the checkpoints written afterwards
    was_training = routine.training
    routine.eval()
    try:
        with torch.no_grad():
            if kind == "markov" and "data" not in batch:      # one-step pairs
                return float(routine.pair_loss(batch).item())
            # (Markov trajectory batch: the reference's valid_loss, over the autoregressive rollout, :392-403)
            out = routine.validation_step(batch)
            return float(out["valid_loss"] if isinstance(out, dict) else out)
    finally:
        routine.train(was_training)


def _trial_dir(config_dir: Path, trial: int, checkpoint_id: Optional[str], create: bool) -> Path:
    root = config_dir / "checkpoints"
    found = sorted(root.glob(f"trial-{trial}-*"))
    if checkpoint_id:
        d = root / f"trial-{trial}-{checkpoint_id}"
    elif found:
        d = found[-1]
    else:
        d = root / f"trial-{trial}-{time.strftime('%Y%m%d-%H%M%S')}"
    if create:
        d.mkdir(parents=True, exist_ok=True)
    return d


def _best_checkpoint(config_dir: Path, trial: int, explicit: Optional[str]) -> Path:
    if explicit:
        return Path(explicit)
    paths = sorted((config_dir / "checkpoints").glob(f"trial-{trial}-*/epoch*.ckpt"))
    if len(paths) != 1:      # the reference asserts exactly one (commands/test.py:56-60)
        raise FileNotFoundError(f"expected exactly one checkpoints/trial-{trial}-*/epoch*.ckpt under {config_dir}, "
                                f"found {len(paths)}")
    return paths[0]


# ------------------------------------------------------------------------------------------------------------------
@app.command()
def train(config_path: Path, overrides: Optional[List[str]] = Argument(None), force: bool = False, resume: bool = False,
          checkpoint_id: Optional[str] = None, trial: int = 0, debug: bool = False, no_logging: bool = False,
          steps: int = Option(20, help="optimisation steps to run (the reference runs trainer.max_epochs epochs)"),
          accumulation_batches: int = Option(4, help="epoch-0 batches that only accumulate the normaliser statistics"),
          steps_per_epoch: int = Option(0, help="advance the epoch counter (StepLR, file names) every N steps; 0 = never"),
          data: Optional[Path] = Option(None, help=".npz with the builder's batch arrays; default: synthetic fields"),
          valid_data: Optional[Path] = Option(None, help="Markov routine: .npz of whole trajectories (data [n, M, N, T] [, times, "
                                                         "f, mu, corr_data]); valid_loss becomes the trajectory loss of "
                                                         "validation_step over its first batch"),
          batch_size: Optional[int] = None, grid: int = 64, size: Optional[List[int]] = Option(None, help="mesh size"),
          epochs: int = Option(0, help="trajectory training file: run this many whole epochs instead of --steps"),
          no_shuffle: bool = Option(False, "--no-shuffle", help="trajectory training file: pairs in (b t) order, not a permutation "
                                                                "per epoch"),
          drop_last: bool = Option(False, "--drop-last", help="trajectory training file: drop the short last batch of an epoch"),
          pair_stride: Optional[int] = Option(None, help="trajectory training file: steps k between a pair's input and target "
                                                         "(default 1)"),
          pair_mode: Optional[str] = Option(None, help="trajectory training file: ns_markov (inputs k ... T-1-k, with dx / dy; the "
                                                       "default) or kolmogorov (inputs 0 ... T-1-k)"),
          builder: bool = Option(False, "--builder", help="train on the dataset files of the config's `builder` section "
                                                          "(StructuredMesh2DBuilder, PlasticityBuilder, ElasticityBuilder, "
                                                          "NSMarkovBuilder, NSZongyiBuilder, NSContextualBuilder, KolmogorovBuilder) for --epochs (default "
                                                          "trainer.max_epochs) whole epochs, validating on the held-out split after "
                                                          "each; the Markov routine's epoch 0 only accumulates its normaliser"),
          device: Optional[str] = Option(None, hidden=True)):
    """Train: build the routine from CONFIG (+ `a.b=c` overrides) and run fused optimisation steps."""
    cfg = load_config(str(config_path), overrides or [])
    rank, world, dev = _init_distributed(device)
    torch.manual_seed(int(cfg.get("seed", 7231 + trial)))      # commands/train.py:61-64 (the same initial weights on every rank)
    routine = build_routine(cfg).to(dev)
    _LAST["routine"] = routine
    kind = routine_kind(routine)
    if kind == "pointcloud" and world > 1:
        raise NotImplementedError("PointCloudExperiment: data parallel training is not built (one process, one GPU)")
    run = SimpleNamespace(cfg=cfg, routine=routine, kind=kind, dev=dev, rank=rank, world=world, config_path=config_path, trial=trial,
                          checkpoint_id=checkpoint_id, no_logging=no_logging, force=force, resume=resume)
    if builder:
        if data is not None or steps_per_epoch:
            raise ValueError("--builder takes its batches from the config's builder section and runs whole epochs: it goes with "
                             "neither --data nor --steps-per-epoch")
        if epochs < 0:
            raise ValueError("--epochs is a positive number of whole epochs")
        return _train_from_builder(run, epochs, no_shuffle, drop_last, batch_size)
    # a trajectory file is trained on when the command says how: any of the options below selects the pair rule and the epoch
    # order (each has a default); without one of them the file is refused as before
    as_trajectories = bool(epochs or no_shuffle or drop_last or pair_stride is not None or pair_mode is not None)
    if as_trajectories:
        if kind != "markov" or data is None or not holds_trajectories(data):
            raise ValueError("--epochs, --no-shuffle, --drop-last, --pair-stride and --pair-mode need a trajectory training file: "
                             "the Markov routine with --data FILE holding data [n, M, N, T]")
        if epochs < 0 or (epochs and steps_per_epoch):
            raise ValueError("--epochs is a positive number of whole epochs and sets the epoch length itself (no --steps-per-epoch)")
        batches = trajectory_batches(routine, cfg, dev, data, batch_size, pair_mode or "ns_markov", 1 if pair_stride is None else pair_stride,
                                      seed=7231 + trial, shuffle=not no_shuffle, drop_last=drop_last, rank=rank, world=world)
        if epochs:
            steps, steps_per_epoch = epochs * len(batches), len(batches)
    else:
        batches = Batches(routine, cfg, dev, data, batch_size, grid, size, seed=7231 + trial, rank=rank, world=world)
        if batches.trajectories:
            raise ValueError(f"{data}: a trajectory file cannot be trained on as it is (training takes x / y pairs); pass it as "
                             f"--valid-data, or say how pairs are drawn from it: --pair-mode ns_markov|kolmogorov (or any of "
                             f"--pair-stride, --epochs, --no-shuffle, --drop-last)")
    valid_batch = None
    if valid_data is not None:
        if kind != "markov":
            raise ValueError("--valid-data takes the Markov routine's trajectory files; the other routines validate on --data")
        valid = Batches(routine, cfg, dev, valid_data, batch_size, grid, size, seed=7231 + trial)
        if not valid.trajectories:
            raise ValueError(f"{valid_data}: no `data` [n, M, N, T] array (found {sorted(valid.arrays)})")
        valid_batch = next(iter(valid))
    out_dir, start = _open_run(run)
    it = iter(batches)
    epoch = start["epoch"]
    if kind == "markov" and not resume and routine.should_normalize:      # epoch 0: statistics only (:376-378)
        for _ in range(accumulation_batches):
            routine.training_step(next(it), epoch=0)
        epoch = max(epoch, 1)
    if epochs:      # whole epochs from here on: what the statistics pass left of its epoch is not trained on
        it = iter(batches)
    routine.current_epoch = epoch
    t0 = _now(dev)
    loss = None
    for step in range(steps):
        loss = _train_step(routine, kind, next(it), epoch, step)
        if steps_per_epoch and (step + 1) % steps_per_epoch == 0:
            epoch += 1
            if hasattr(routine, "on_train_epoch_end"):
                routine.on_train_epoch_end()
            else:      # the Markov routine: told the epoch by every training_step
                routine.current_epoch = epoch
        if step % max(1, steps // 5) == 0 or step == steps - 1:
            lv = float(loss.item())
            if not math.isfinite(lv):
                # activations, spectra and gradients are range-safe by construction (include/ffno.h "Range words"); what is left is
                # data that is non-finite already, a diverged run, or WEIGHTS beyond the half format's range in the split-fp16
                # packs (|W| >= 65504) -- the any-range arithmetic is one switch away
                raise FloatingPointError(
                    f"non-finite training loss at step {start['global_step'] + step}: check the data and the learning rate; if the "
                    f"weights have grown past 6.5e4, run with FFNO_FF_SPLIT=bf16x3 FFNO_X3_MIX_SPLIT=bf16x3 (any fp32 range)")
            if rank == 0:
                print(json.dumps(dict(step=start["global_step"] + step, epoch=epoch, train_loss=round(lv, 6),
                                      lr=routine.trainer().current_lr())), flush=True)
    dt = _now(dev) - t0
    summary = dict(steps=steps, batch=batches.B if isinstance(batches, Batches) else batches.batch_size, world_size=world,
                   **(dict(epochs=epochs) if epochs else {}), steps_per_s=round(steps / max(dt, 1e-9), 2),
                   resumed_from_step=start["global_step"])
    if out_dir is not None:
        gs = start["global_step"] + steps
        vl = _valid_loss(routine, kind, valid_batch if valid_batch is not None else next(it))
        for old in out_dir.glob("epoch*.ckpt"):      # CustomModelCheckpoint keeps the single best file
            old.unlink()
        best = out_dir / f"epoch={epoch}-step={gs}-valid_loss={vl:.5f}.ckpt"
        routine.save_checkpoint(str(best), epoch=epoch, global_step=gs)
        routine.save_checkpoint(str(out_dir / "last.ckpt"), epoch=epoch, global_step=gs)
        summary.update(valid_loss=round(vl, 6), checkpoint=str(best))
    if rank == 0:
        print(json.dumps(summary), flush=True)
    if world > 1:
        torch.distributed.barrier()


@app.command()
def test(config_path: Path, overrides: Optional[List[str]] = Argument(None), force: bool = False, trial: int = 0,
         map_location: Optional[str] = None, debug: bool = False, no_logging: bool = False,
         batches: int = Option(1, help="test batches to average over"), data: Optional[Path] = None,
         batch_size: Optional[int] = None, grid: int = 64, size: Optional[List[int]] = None,
         builder: bool = Option(False, "--builder", help="the test metrics over the whole test split of the config's `builder` "
                                                         "section (KolmogorovBuilder: with test_reduced_time_until, on the grid "
                                                         "of its corr_data)"),
         pred_path: Optional[Path] = Option(None, "--pred-path", help="write the test predictions of a Markov routine here (vorticity, "
                                                                      "vx, vy on the routine's pred_size grid and their energy "
                                                                      "spectrum, as the .npz sibling of the path): overrides the "
                                                                      "config's routine.pred_path"),
         device: Optional[str] = Option(None, hidden=True)):
    """Test: load the best checkpoint of the trial (or `checkpoint_path=...` override) and report the test metrics.  A Markov
    routine with a pred_path (the torus_kochkov/ffno/predictions configs, or --pred-path) also writes its predictions, one file
    for all test batches, and reports `pred_path` (the file written) and `pred_samples`."""
    if builder and data is not None:
        raise ValueError("--builder takes the test split from the config's builder section: it does not go with --data")
    cfg, routine, kind, ckpt = _load_trained(config_path, overrides, trial, map_location, device)
    dev = _device(device)
    if pred_path is not None:
        if kind != "markov":
            raise ValueError(f"--pred-path writes the test predictions of Grid2DMarkovExperiment; this config's routine is "
                             f"{type(routine).__name__}")
        routine.pred_path = str(pred_path)
    parts = _PredictionParts(routine) if getattr(routine, "pred_path", None) is not None else None
    if builder:
        bld = _instantiate_builder(cfg, kind, batch_size, routine)
        test_set = bld.test_data(dev)
        if kind in TEST_KEYS:
            reduced = ("test_reduced_time_until",) if type(bld).__name__ == "KolmogorovBuilder" else ()
            m = _split_loss(routine, test_set, "test_step", TEST_KEYS[kind] + reduced, each=parts)
        else:
            m = dict(test_loss=_split_loss(routine, test_set)["valid_loss"])
        written = parts.write() if parts is not None else {}
        print(json.dumps(dict(checkpoint=str(ckpt), **{k: round(v, 6) for k, v in m.items()}, samples=test_set.n, **written)),
              flush=True)
        return
    src = Batches(routine, cfg, dev, data, batch_size, grid, size, seed=7231 + trial)
    if parts is not None and not src.trajectories:      # one-step pairs or synthetic fields: test_step, which exports, does not run
        if pred_path is not None:
            raise ValueError("--pred-path: the predictions come from the trajectory rollout of test_step; give `--data TRAJ.npz` "
                             "holding data [n, M, N, T], or --builder")
        parts = None
    it = iter(src)
    acc: Dict[str, float] = {}
    for _ in range(batches):
        b = next(it)
        if kind == "rollout" or src.trajectories:      # (trajectories: the reference's test metrics of the Markov routine, :408-416)
            out = routine.test_step(b)
            if parts is not None:
                parts(out)
            m = {k: v for k, v in out.items() if k in TEST_KEYS[kind]}
        else:
            m = {"test_loss": _valid_loss(routine, kind, b)}
        for k, v in m.items():
            acc[k] = acc.get(k, 0.0) + float(v) / batches
    written = parts.write() if parts is not None else {}
    print(json.dumps(dict(checkpoint=str(ckpt), **{k: round(v, 6) for k, v in acc.items()}, **written)), flush=True)


@app.command()
def predict(config_path: Path, overrides: Optional[List[str]] = Argument(None), trial: int = 0,
            map_location: Optional[str] = None, debug: bool = False,
            n_steps: Optional[int] = Option(None, help="rollout length (default: the routine's n_steps)"),
            output: Optional[Path] = Option(None, help="write the predictions here (.npz); default: <trial dir>/predictions.npz"),
            data: Optional[Path] = None,
            batch_size: Optional[int] = Option(None, help="default 1; with --builder: trajectories per chunk, default all at once"),
            grid: int = 64, size: Optional[List[int]] = None,
            builder: bool = Option(False, "--builder", help="Markov and rollout routines: predict on the `inference_data()` of the "
                                                            "config's `builder` section (the first 512 trajectories of its file; "
                                                            "KolmogorovBuilder: its test trajectories) "
                                                            "and report the reference's `inference_time`"),
            device: Optional[str] = Option(None, hidden=True)):
    """Predict: load the best checkpoint, run the model autoregressively (grid routines) or once (mesh routine), save the
    predictions and report the time per model step (the reference's `inference_time`, commands/train.py:132-148)."""
    if builder and data is not None:
        raise ValueError("--builder takes the trajectories from the config's builder section: it does not go with --data")
    cfg, routine, kind, ckpt = _load_trained(config_path, overrides, trial, map_location, device)
    dev = _device(device)
    traj = None
    if builder:
        if kind not in TEST_KEYS:
            raise ValueError("predict --builder runs the Markov and rollout routines (NSMarkovBuilder, NSZongyiBuilder, KolmogorovBuilder), whose "
                             "builders have inference_data()")
        bld = _instantiate_builder(cfg, kind, None, routine)
        if not hasattr(bld, "inference_data"):
            raise ValueError(f"predict --builder runs on a builder's inference_data(), and {type(bld).__name__} has none -- the "
                             f"reference gives it none either (builders/ns_contextual.py): use `test --builder` for its test "
                             f"split, or `rollout --init FILE` to run the model as a simulator")
        traj = bld.inference_data(dev)["data"]
        chunk = batch_size or len(traj)
        if chunk < 1:
            raise ValueError("--batch-size is at least 1")
    else:
        b = next(iter(Batches(routine, cfg, dev, data, batch_size or 1, grid, size, seed=7231 + trial)))

    def run():
        with torch.no_grad():
            if traj is not None:      # commands/train.py:134-143: routine.infer over the trajectories, here --batch-size at a time
                parts = []
                for lo in range(0, len(traj), chunk):
                    part = {"data": traj[lo:lo + chunk]}
                    # (_valid_step here and _learning_step below: the routines' own names for the prediction pass; the one
                    # place the commands reach for an underscore-prefixed member of a routine)
                    parts.append(routine._valid_step(part)[2] if kind == "markov" else routine.forward(part)[2])
                return parts[0] if len(parts) == 1 else torch.cat(parts)
            if kind == "markov":
                return routine.rollout(b["x"], n_steps, b.get("f"), b.get("mu"))
            if kind == "rollout":
                return routine._learning_step(b)[2]
            if kind == "pointcloud":
                return routine(b)
            return routine.trainer().predict(b["x"])

    run()       # warm-up (routine.warmup() in the reference)
    t0 = _now(dev)
    preds = run()
    elapsed = _now(dev) - t0
    steps = (n_steps or getattr(routine, "n_steps", None) or 1) if kind not in ("mesh", "pointcloud") else 1
    out = output or (ckpt.parent / "predictions.npz")
    np.savez(str(out), preds=preds.detach().cpu().numpy())
    extra = {}
    if traj is not None:      # the reference's own figure: seconds per trajectory and unit of simulated time (commands/train.py:144-148)
        steps = routine.n_steps or traj.shape[-1] - 1
        extra = dict(samples=len(traj), n_steps=steps, step_size=routine.step_size, elapsed=elapsed,
                     inference_time=elapsed / len(traj) / (routine.step_size * steps))
    print(json.dumps(dict(checkpoint=str(ckpt), predictions=str(out), shape=list(preds.shape),
                          inference_time_ms_per_step=round(1e3 * elapsed / steps, 4), **extra)), flush=True)


@app.command()
def rollout(config_path: Path, overrides: Optional[List[str]] = Argument(None), trial: int = 0,
            map_location: Optional[str] = None,
            init: Path = Option(..., help=".npz of initial conditions: x0, vorticity or data as [n, M, N] (a trajectory array "
                                          "[n, M, N, T] gives its first time slice) [, f [n, M, N] or [n, M, N, >= steps], mu [n]]"),
            steps: int = Option(100, help="model steps to simulate"),
            every: int = Option(1, help="keep every N-th state (divides --steps)"),
            batch_size: Optional[int] = Option(None, help="samples simulated at once; default: the whole file"),
            output: Optional[Path] = Option(None, help="write preds and times here (.npz); default: <trial dir>/rollout.npz"),
            device: Optional[str] = Option(None, hidden=True)):
    """Rollout: load the best checkpoint and run the model as a simulator from the initial conditions of --init (the reference's
    `fourierflow infer`, commands/infer.py): `preds` [n, M, N, steps / every] and `times` = step_size * every * (1 .. L), one
    warm-up chunk, then the timed run; reports ms per model step and the reference's `inference_time` (seconds per sample and
    unit of simulated time)."""
    arrays = {}

    def accept(routine, kind):
        if kind != "markov":
            raise ValueError(f"rollout runs the Markov routine (Grid2DMarkovExperiment); this config builds {type(routine).__name__}")
        if batch_size is not None and batch_size < 1:
            raise ValueError("--batch-size is at least 1")
        if steps < 1 or every < 1 or steps % every:
            raise ValueError(f"--steps is a positive multiple of --every, got --steps {steps} --every {every}")
        arrays.update(initial_conditions(init, routine))

    _, routine, _, ckpt = _load_trained(config_path, overrides, trial, map_location, device, accept)
    dev = _device(device)
    n = len(arrays["x0"])
    chunk = min(batch_size or n, n)
    on_dev = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}

    def run(lo):
        part = {k: v[lo:lo + chunk] for k, v in on_dev.items()}
        return routine.simulate(part["x0"], steps, part.get("f"), part.get("mu"), every=every)

    run(0)      # warm-up: workspaces, weight packs
    t0 = _now(dev)
    parts = [run(lo) for lo in range(0, n, chunk)]
    elapsed = _now(dev) - t0
    preds = parts[0] if len(parts) == 1 else torch.cat(parts)
    finite = bool(torch.isfinite(preds[..., -1]).all().item())      # the final field: one host read
    out = output or (ckpt.parent / "rollout.npz")
    L = preds.shape[-1]
    np.savez(str(out), preds=preds.cpu().numpy(),
             times=(routine.step_size * every * np.arange(1, L + 1)).astype(np.float32))
    print(json.dumps(dict(checkpoint=str(ckpt), predictions=str(out), shape=list(preds.shape), steps=steps, every=every,
                          samples=n, batch=chunk, step_size=routine.step_size, elapsed=elapsed,
                          ms_per_step=round(1e3 * elapsed / (steps * len(parts)), 4), finite=finite,
                          inference_time=elapsed / n / (routine.step_size * steps))), flush=True)


# ------------------------------------------------------------------------------------------------------------------
generate_app = Typer(add_completion=False, help="Generate datasets on the GPU.")
app.add_typer(generate_app, name="generate")


@generate_app.callback()
def _generate():
    """Generate datasets on the GPU (the reference's `fourierflow generate`, commands/generate.py)."""


@generate_app.command("navier-stokes")
def navier_stokes(path: str = Argument(..., help="prefix of the files to write: PATH.train.npz, PATH.valid.npz, PATH.test.npz"),
                  n_train: int = Option(1000, help="trajectories in PATH.train.npz"),
                  n_valid: int = Option(200, help="trajectories in PATH.valid.npz"),
                  n_test: int = Option(200, help="trajectories in PATH.test.npz"),
                  s: int = Option(256, help="grid points per side (a power of two, 8 ... 512)"),
                  t: float = Option(20, help="time the flow is integrated to"),
                  steps: int = Option(20, help="snapshots kept per trajectory, evenly spaced up to --t"),
                  mu: float = Option(1e-5, help="viscosity of every trajectory when --mu-min equals --mu-max"),
                  mu_min: float = Option(1e-5, help="lower end of the per-trajectory uniform viscosity"),
                  mu_max: float = Option(1e-5, help="upper end of the per-trajectory uniform viscosity"),
                  seed: int = Option(23893, help="seeds torch (initial vorticity) and, plus 1234, numpy (viscosity, force)"),
                  delta: float = Option(1e-4, help="time step of the solver"),
                  batch_size: int = Option(50, help="trajectories solved at once"),
                  force: Force = Option(Force.li.value, help="forcing term of the vorticity equation"),
                  cycles: int = Option(2, help="--force random: harmonics per direction"),
                  scaling: float = Option(0.1, help="--force random: factor on the summed harmonics"),
                  t_scaling: float = Option(0.2, help="--varying-force: the phase of the force is this times the time"),
                  varying_force: bool = Option(False, "--varying-force",
                                               help="--force random: advance the phase of the force with time, and write one "
                                                    "force map per snapshot"),
                  ssr: int = Option(1, help="keep every ssr-th grid point of the solutions (the builders' stride subsampling)"),
                  train_trajectories: bool = Option(False, "--train-trajectories",
                                                    help="write PATH.train.npz as whole trajectories like the other two splits "
                                                         "(`train --data` draws its pairs from them on the device)"),
                  device: Optional[str] = Option(None, hidden=True)):
    """Generate 2-D Navier-Stokes trajectories (the reference's `fourierflow generate navier-stokes`: GaussianRF initial vorticity,
    the Crank-Nicolson solver, the same options and seeding) and write them as the .npz files `train` / `test` / `predict` read:
    PATH.train.npz holds x / y pairs [, f, mu] (with --train-trajectories: whole trajectories like the other two), PATH.valid.npz
    and PATH.test.npz whole trajectories data [n, M, N, T], times [, f, mu].  `f` is written for --force random, `mu` when
    --mu-min and --mu-max differ.  With --varying-force (the `torus_vis_force` data) the random force gets the phase
    --t-scaling times the time, a new field at every solver step, and `f` holds one map per snapshot: [n, M, N, steps] beside `data`
    (column i is the force of the step that gave data[..., i]), and in the x / y form the map of each pair's y.  Each split is solved --batch-size trajectories at a time, with a shorter last batch where that does not divide the split, and written batch by batch."""
    from .builders.synthetic import generate_navier_stokes
    if steps < 2:
        raise BadParameter("a training pair needs two snapshots", param_hint="--steps")
    if batch_size < 1 or ssr < 1:
        raise BadParameter("--batch-size and --ssr are at least 1")
    if varying_force and force != Force.random:
        raise BadParameter("--varying-force goes with --force random (the only force with a phase to advance)", param_hint="--varying-force")
    if varying_force and not 1 <= cycles < s // 2:
        raise BadParameter(f"--varying-force: 1 <= cycles < s / 2 = {s // 2}", param_hint="--cycles")
    summary = generate_navier_stokes(path, _device(device), n_train=n_train, n_valid=n_valid, n_test=n_test, s=s, t=t, steps=steps, mu=mu,
                                     mu_min=mu_min, mu_max=mu_max, seed=seed, delta=delta, batch_size=batch_size, force=force,
                                     cycles=cycles, scaling=scaling, ssr=ssr, train_trajectories=train_trajectories, t_scaling=t_scaling,
                                     varying_force=varying_force)
    print(json.dumps(summary), flush=True)


@generate_app.command("kolmogorov")
def kolmogorov(config_path: Path = Argument(..., help="a data-generation YAML of the reference's data/kolmogorov tree"),
               overrides: Optional[List[str]] = Argument(None, help="a.b=c overrides of the YAML, e.g. sim_grid.shape=[256,256]"),
               batch_size: int = Option(1, help="trajectories solved at once"),
               device: Optional[str] = Option(None, hidden=True)):
    """Generate 2-D Kolmogorov flows (the reference's `fourierflow generate kolmogorov`): the pseudo-spectral solver with
    Crank-Nicolson / RK4 time stepping, Kolmogorov forcing and drag that CONFIG describes, written beside CONFIG as the .npz files
    KolmogorovBuilder reads in place of the reference's .nc files.  With warmup_steps > 0 (the initial_conditions files): the
    final fields, STEM_{size}.npz holding vorticity [n, size, size].  Otherwise (the trajectories files, started from
    `init_path`): STEM_{size}_{k}.npz holding vorticity [n, outer_steps // k, size, size], every k-th snapshot starting at the
    k-th, and time.  Sizes below the simulation grid are reduced through the staggered velocity, as the reference does."""
    from .builders.kolmogorov_flow import generate_kolmogorov, plan_kolmogorov
    if batch_size < 1:
        raise BadParameter("--batch-size is at least 1")
    plan = plan_kolmogorov(load_config(str(config_path), overrides or []), str(config_path))
    t0 = time.perf_counter()
    written = generate_kolmogorov(plan, _device(device), batch_size)
    print(json.dumps(dict(dt=plan.dt, steps=plan.solver_steps, grid=plan.N, trajectories=plan.n_trajectories,
                          elapsed=time.perf_counter() - t0, files=written)), flush=True)


def main():
    app()


if __name__ == "__main__":
    main()
