"""Host-side driver of the F-FNO block: sequences the C-ABI kernels of include/ffno.h.

Mirrors the data flow of the reference's ``FNOFactorized2DBlock.forward``
(fourierflow/modules/factorized_fno/grid_2d.py:154-177), of the 3-D mesh variant
``FNOFactorizedMesh3D.forward`` (mesh_3d.py:160-176) and of their autograd, over pre-allocated device
workspaces and raw pointers:

  forward :  lift -> L x [ per axis: DFT -> mode mix -> iDFT (+sum) ; fused FF (+residual) ] -> head
  backward:  head_bwd -> L x [ ff_bwd_data, ff_bwd_weights, per axis: adjoint DFT/mix/iDFT accumulating into
             the running gradient ] -> lift_bwd -> Fourier-weight gradients (one launch per weight over all
             layers) -> weight-norm backward (one batched launch)

Every spatial axis is a *view* of the channels-last activation buffer as [B', M', N', C] plus a flag saying
whether the transform runs along N' (contiguous lines) or M' (strided lines), so the same spectral kernels
serve the 2-D grid (2 axes) and the 3-D mesh (3 axes, any sizes incl. the +8 padding).

PyTorch is used for device memory and the stream only.  All parameter gradients land in one flat
fp32 buffer (``gflat``) so the trainer can run ONE fused AdamW and ONE RCCL all-reduce per step.
"""
from __future__ import annotations

import collections
import ctypes
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi, _lib
from ._corner_chain import CornerChain
from ._engine_core import EngineCore

_p = _lib.ptr

MODES = {"full": 0, "low-pass": 1, "no-fourier": 2}
HEAD_DIM = 128  # grid_2d.py:150-152 / mesh_3d.py:155-157: WNLinear(width, 128) -> WNLinear(128, out)
_SUPPORTED_CH = {(64, 256), (64, 128), (32, 128), (32, 64)}      # = what ffno_ffx_supported takes (csrc/ffx.hip FFNO_FX_DISPATCH)
# paired spectral launch, workgroup -> (branch, tile) map (ffno_spectral_x3_pair `interleave`): bit 1 = image-local where the shapes
# allow it (the workgroups that read one image share an XCD, so the image crosses HBM once: PMC traffic 178.9 -> 150.7 MB per launch,
# round 2), else bit 0 = even workgroups branch a, odd ones branch b
X3_INTERLEAVE = 3
# all-layers feed-forward weight-gradient launch: rounds of resident workgroups (FF_WGRAD_ROUNDS x CUs / L slices per layer)
FF_WGRAD_ROUNDS = 3
# workgroups of a Fourier-weight-gradient launch (slices x modes; with per-layer weights slices x modes x layers)
FW_GRAD_WGS = 512
# workspaces an engine keeps, one per (batch, grid, saving) geometry, least recently used dropped first.  A run over two grid sizes
# visits six between two checkpoints -- the full training batch of either size, the short last one, the full and the short
# validation batch and the test / predict batch -- and must not allocate in the steady state; with four, kept first-in first-out
# as before, every epoch of such a run dropped and rebuilt its training workspaces.
WS_CACHE_MAX = 8


def _fmix32(h: int) -> int:
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _site_seed(*words: int) -> int:
    """Seed of one dropout site: a hash CHAIN over (base seed, training call, layer, linear, block kind), not a linear
    combination of them -- linear seeds made the masks of neighbouring sites shifted copies of one sequence."""
    h = 0x9E3779B1
    for w in words:
        h = _fmix32(h ^ _fmix32((int(w) + 0x7F4A7C15) & 0xFFFFFFFF))
    return h


class _StackRetry(Exception):
    """The first persistent inference launch of a workspace reported an error: forward() starts over on the per-layer launches."""


class _Plan(NamedTuple):
    """What one forward pass (and the backward pass over it) runs, decided once before the layer loop."""
    fused: List[bool]         # per axis: a fused branch kernel (else the stage kernels)
    x3: List[bool]            # per axis: ... on the split (x3) fused kernels
    x3fmt: List[int]          # per axis: format of the packed x3 weight sets (ffno.h FFNO_PLANES_*)
    singles: List[int]        # axes that run on their own launches
    pair: Optional[Tuple[int, int]]      # the two axes that share paired launches
    conc: bool                # pair is not None
    x3pair: bool              # the paired launches run on the split kernels
    layer_calls: bool         # forward: one ffno_layer_fwd call per layer
    bwd_layer_calls: bool     # backward: one ffno_layer_bwd call per layer (unless a timer is attached by then)
    infer: bool               # the two-launch inference layer
    infer_sr: bool            # ... self-ranged (no range words in this pass)
    lazy: bool                # the feed-forward input sums are left to the deferred weight-gradient launch
    bf16: bool                # bf16 activation storage
    save: bool                # the pass saves for a backward pass


# what forward(save_for_backward=True) hands to backward(): its input, the workspace it filled (and that workspace's key), its plan
_Saved = collections.namedtuple("_Saved", "x B S ws ws_key plan")


class _Linear:
    __slots__ = ("prefix", "rows", "cols", "wnorm", "weff", "gweff", "fx")

    def __init__(self, prefix, rows, cols, wnorm):
        self.prefix, self.rows, self.cols, self.wnorm = prefix, rows, cols, wnorm
        self.weff = None   # effective weight [rows, cols] (after weight-norm)
        self.gweff = None  # gradient w.r.t. the effective weight
        self.fx = None     # the four operand packs of the feed-forward block this linear belongs to (forward A1/A2, backward A1/A2)


class _View:
    """One spatial axis as a [Bv, Mv, Nv, C] view: a01 = 0 transforms along Nv, 1 along Mv."""
    __slots__ = ("Bv", "Mv", "Nv", "a01", "L", "K", "R", "spec", "modes", "x3fmt")

    def __init__(self, Bv, Mv, Nv, a01, K, C):
        self.Bv, self.Mv, self.Nv, self.a01, self.K = Bv, Mv, Nv, a01, K
        self.L = Nv if a01 == 0 else Mv
        self.R = Bv * Mv if a01 == 0 else Bv * Nv
        self.spec = K * self.R * 2 * C
        self.modes = K      # what the mix and the weight gradient run over
        self.x3fmt = None   # format of the packed x3 weight set this axis reads (ffno.h FFNO_PLANES_*): set by every pass's plan


class _DeferredWord:
    """One device word that is looked at a round late: copied to pinned host memory behind the work in flight, with an event
    recorded after the copy, and read the next time round once the event has passed -- no synchronisation."""

    def __init__(self, device):
        self.host = torch.zeros(1, dtype=torch.int32)
        if device is not None and device.type == "cuda":
            self.host = self.host.pin_memory()
        self.event = None
        self.pending = False

    def post(self, word: torch.Tensor):
        """Start the copy of ``word`` (one int32 on the device) on the current stream."""
        self.host.copy_(word, non_blocking=True)
        self.event = torch.cuda.Event() if word.is_cuda else None      # (the emulator backend: the copy is done by now)
        if self.event is not None:
            self.event.record()
        self.pending = True

    def take(self) -> Optional[torch.Tensor]:
        """The host copy, once, when a posted copy has landed; None while there is nothing new to look at."""
        if not self.pending or (self.event is not None and not self.event.query()):
            return None
        self.pending = False
        return self.host


class _Workspace:
    """The device buffers and per-geometry schedule decisions of one (batch, grid, save) key, every field named once.  A field the
    configuration does not need stays None.  (A plain class, not __slots__: bench.py and tools/power_trace.py walk a workspace's
    tensors through vars().)"""

    def __init__(self):
        self.P = self.P_in = None        # pixels of the (padded) activation buffers / of the inputs and outputs
        self.Sp = None                   # padded grid
        self.views = None                # one _View per spatial axis (spectral="plus": the one CornerChain)
        self.padmap = self.pm = None     # _capi.PadMap of a padded operator, and byref() of it: the argument the kernels take
        self.X = None                    # running activation
        self.Blast = None                # the last layer's output (head input)
        self.Y = None                    # head output
        self.S = None                    # feed-forward inputs (spectral-branch outputs), per saved layer
        self.SXall = self.SDall = None   # forward / adjoint spectra, per axis, layer-major (kept for the Fourier-weight gradient)
        self.SY = self.SD = None         # scratch spectra of the staged path (mixed / stage-A)
        self.SY2 = self.SD2 = None       # ... of the second branch of a paired STAGE launch
        self.T = self.G1 = None          # output of the second branch of a paired launch / of the second adjoint branch
        self.TS = None                   # lazy sums: the second branch output of every layer
        self.chain = self.scr = None     # spectral="plus": the corner chain (= views[0]) and its scratch
        self.mask_words = None           # int32 words of one layer's packed ReLU sign bits
        # range words, one per (tensor kind, layer): x = layer inputs, s = spectral-branch outputs (feed-forward inputs),
        # g = running gradient (both buffers), d = feed-forward data gradients, t / f = LayerNorm / fork-head gradients
        self.rw_kinds = self.RW = None
        self.rw_bwd_clean = False        # the backward's words are still zero from the forward's clearing launch
        self.TL = self.LNS = None        # LayerNorm: feed-forward outputs before it; {mean, rstd} per pixel
        self.TLF = self.LNSF = None      # ... of the forecast feed-forwards (they end in their own LayerNorm, feedforward.py:18-19)
        self.DT = self.DTF = None        # LayerNorm backward: gradients before it (backcast / forecast)
        self.lnpart = None               # ... its partial slices
        self.F = self.YL = None          # fork heads: forecast_ff outputs f_l (inputs of the shared head); per-layer head outputs
        self.MASKF = self.DSF = None     # fork heads, backward: sign bits, data gradient
        self.GF = self.redl = None       # ... head gradient, per-layer head reduction
        self.HG = None                   # general feed-forward: kept hidden activations per block kind / saved layer / hidden layer
        self.DA = self.glpart = None     # ... backward: ping-pong hidden gradients, weight-gradient slices
        self.MASK = None                 # packed ReLU sign bits per saved layer
        self.DS = None                   # feed-forward data gradient
        # running gradient: a ping-pong pair -- or one buffer per layer when the weight-gradient launches are deferred to the end
        # of the pass (they read every layer's summed gradient then)
        self.G = self.defer_wgrad = None
        self.lazy_sums = None            # "s": the chain kernels leave their input sums to the deferred weight-gradient launch
        self.nsplit_ff = self.nsplit_ffm = None      # feed-forward weight gradient: slices per layer launch / of the all-layers launch
        self.ffpart = None               # ... its partial sums
        # split-bf16 path with per-layer feed-forwards: every layer keeps its own slices and ONE batched launch reduces them all
        # at the end of the backward pass (24 kernel boundaries less per step)
        self.defer_reduce = self.ffparts = None
        self.wg_jobs = self.wg_table = None      # rows of the deferred weight-gradient launch in this backward pass (None: per layer); its table
        self.red_jobs = self.red_table = None    # rows of the batched reduce launch in this backward pass; its table
        self.nsplit_fw = self.fwpart = None      # Fourier-weight gradient: slices per axis, partial sums per (weight set, axis)
        # ... per-layer weights, per axis: partial sums, device table of the layers' gradient pointers, the pointers it was built from
        self.fwpart_multi = self.fwgrad_tab = self.fwgrad_sig = None
        self.nsplit_lift = self.liftpart = None      # lift weight gradient: slices, partial sums
        self.nsplit_head = self.headpart = None      # head weight gradient: slices, partial sums
        self.red = None                  # ... its reduction
        self.MIX = None                  # inference layer: the mixed spectra of the two axes
        self.stack_sync = None           # persistent inference stack: barrier words (the last one is the error word)
        self.stack_late = None           # ... its late look at that word (_DeferredWord)
        self.stack_checked = False       # ... the first launch was checked
        self.stack_calls = 0             # ... launches so far


class FFNOEngine(EngineCore):
    """Kernel sequencer for one factorized-FNO configuration (fp32).

    spatial_dims = 2: FNOFactorized2DBlock -- fourier_weight[0] mixes the LAST axis, [1] the first
                      (grid_2d.py:68,86); no padding; one output channel.
                      (``first_axis_first``: FNOFactorizedMesh2D -- [0] mixes x, [1] mixes y (mesh_2d.py:71-75,92-96), +8
                      zero padding like the 3-D operator (mesh_2d.py:150,158)).
    spatial_dims = 3: FNOFactorizedMesh3D -- fourier_weight[0,1,2] mix x, y, z (mesh_3d.py:71,86,101);
                      activations zero-padded by ``padding`` at the end of every axis after the lift and
                      cropped before the head (mesh_3d.py:165,173); ``output_dim`` outputs.
    """

    can_return_view = True      # forward(..., own_output=False) exists (FFNOTrainer.train_step)

    def __init__(self, *, modes, width: int, input_dim: int, n_layers: int, factor: int, share_weight: bool,
                 share_fork: bool = False, ff_weight_norm: bool = False, mode: str = "full", spatial_dims: int = 2,
                 padding: int = 0, output_dim: int = 1, use_fork: bool = False, first_axis_first: bool = False,
                 spectral: str = "factorized", layer_norm: bool = False, n_ff_layers: int = 2, dropout: float = 0.0,
                 in_dropout: float = 0.0):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {list(MODES)}, got {mode!r}")
        if spatial_dims not in (2, 3):
            raise ValueError("spatial_dims must be 2 or 3")
        C, H = width, factor * width
        if (C, H) not in _SUPPORTED_CH:
            raise ValueError(f"(width, factor*width)=({C},{H}) is outside the compiled HIP kernel set {_SUPPORTED_CH}")
        if not (0 < input_dim < 64):
            raise ValueError("input_dim must be in 1..63")
        if not (1 <= output_dim <= 8):
            raise ValueError("output_dim must be in 1..8")
        if n_ff_layers < 2:
            raise NotImplementedError("n_ff_layers = 1 (a single width -> width linear) is not built")
        if not (0.0 <= dropout < 1.0 and 0.0 <= in_dropout < 1.0):
            raise ValueError("dropout / in_dropout must lie in [0, 1)")
        # FeedForward beyond the fused kernels' shape (n_layers = 2, dropout = 0; feedforward.py:13-23): the GENERAL path, one
        # glin kernel per linear layer with kept hidden activations and regenerated dropout masks (csrc/glin.hip)
        self.n_ff, self.dropout, self.in_dropout = int(n_ff_layers), float(dropout), float(in_dropout)
        self.general_ff = self.n_ff != 2 or self.dropout > 0.0
        self.drop_seed = int(torch.initial_seed()) & 0x7FFFFFFF      # base seed of the dropout masks (tests may set it)
        # FeedForward(layer_norm=True): nn.LayerNorm(width) after the last linear of every feed-forward (feedforward.py:18-19)
        self.layer_norm = bool(layer_norm)
        if spectral not in ("factorized", "plus", "dct"):
            raise ValueError("spectral must be 'factorized', 'plus' or 'dct'")
        if spectral == "dct" and mode != "full":
            raise ValueError("the DCT operators (CNOFactorized*) have no `mode` switch")
        if spectral == "plus" and (spatial_dims != 2 or padding or mode == "low-pass"):
            raise ValueError("the non-factorized (FNOPlus2DBlock) spectral conv is 2-D, unpadded, mode 'full' or 'no-fourier'")
        # "plus": rfft2 + two K x K corner blocks (zongyi_fno/grid_plus_2d.py:52-83);  "dct": orthonormal DCT-II per axis with
        # real per-mode weights [C, C, K] (CNOFactorized*, factorized_cno/grid_2d.py:51-96)
        self.spectral = spectral
        self.nd = spatial_dims
        # 2-D weight order: grid_2d.py has fourier_weight[0] on the LAST axis; mesh_2d.py has [0] on the FIRST (x) axis
        self.first_axis_first = bool(first_axis_first)
        self.Ks: Tuple[int, ...] = tuple(modes) if isinstance(modes, (tuple, list)) else (int(modes),) * spatial_dims
        if len(self.Ks) != spatial_dims:
            raise ValueError("one mode count per spatial axis")
        self.K = self.Ks[0]
        self.C, self.H, self.Cin, self.L, self.O, self.pad = C, H, input_dim, n_layers, output_dim, padding
        self.mode, self.mode_id = mode, MODES[mode]
        self.share_weight, self.share_fork, self.wnorm = share_weight, share_fork, ff_weight_norm
        self.use_fork = use_fork   # per-layer forecast heads: forecast = sum_l out(forecast_ff_l(s_l))  (grid_2d.py:164-167)
        # every layer is spectral branches + ONE two-linear feed-forward with the residual: what the paired / per-layer-call /
        # deferred / inference schedules are written for
        self._plain_layer = not (use_fork or self.layer_norm or self.general_ff)

        # ---- parameter inventory, in the reference's named_parameters() naming --------------------
        self.linears: Dict[str, _Linear] = {}
        shapes: Dict[str, Tuple[int, ...]] = {}

        def add_linear(prefix, rows, cols):
            if prefix in self.linears:
                return
            self.linears[prefix] = _Linear(prefix, rows, cols, ff_weight_norm)
            if ff_weight_norm:
                shapes[prefix + "weight_g"] = (rows, 1)
                shapes[prefix + "weight_v"] = (rows, cols)
            else:
                shapes[prefix + "weight"] = (rows, cols)
            shapes[prefix + "bias"] = (rows,)
            if layer_norm and prefix.endswith(f"_ff.layers.{self.n_ff - 1}.0."):   # the Sequential slot of the reference: layers.<last>.3
                shapes[prefix[:-2] + "3.weight"] = (rows,)
                shapes[prefix[:-2] + "3.bias"] = (rows,)

        add_linear("in_proj.", C, input_dim)
        self.ff_prefix: List[str] = []
        self.fc_prefix: List[str] = []     # forecast feed-forwards (use_fork)
        self.fw_names: List[Tuple[str, ...]] = []
        def add_ff(prefix):             # FeedForward(dim, factor, ..., n_layers): dims C -> H (-> H)* -> C (feedforward.py:13-16)
            for k in range(self.n_ff):
                add_linear(prefix + f"layers.{k}.0.", C if k == self.n_ff - 1 else H, C if k == 0 else H)

        if share_fork:                      # registration order of the reference: forecast_ff, backcast_ff (grid_2d.py:116-122)
            if use_fork:
                add_ff("forecast_ff.")
            add_ff("backcast_ff.")
        for l in range(n_layers):
            if use_fork:
                fc = "forecast_ff." if share_fork else f"spectral_layers.{l}.forecast_ff."
                self.fc_prefix.append(fc)
                add_ff(fc)
            fp = "backcast_ff." if share_fork else f"spectral_layers.{l}.backcast_ff."
            self.ff_prefix.append(fp)
            add_ff(fp)
            if mode == "full":
                base = "fourier_weight." if share_weight else f"spectral_layers.{l}.fourier_weight."
                names = tuple(base + str(w) for w in range(self.nd))
                self.fw_names.append(names)
                for w, n in enumerate(names):
                    shapes.setdefault(n, (C, C, self.Ks[w], self.Ks[w], 2) if spectral == "plus"
                                      else (C, C, self.Ks[w]) if spectral == "dct" else (C, C, self.Ks[w], 2))
        add_linear("out.0.", HEAD_DIM, C)
        add_linear("out.1.", output_dim, HEAD_DIM)
        self._lay_out(shapes)
        self._fw_sets: List[Tuple[str, ...]] = []   # unique weight tuples in first-use order
        for names in self.fw_names:
            if names not in self._fw_sets:
                self._fw_sets.append(names)
        # weight set of every layer (0 without Fourier weights: no planes are read then)
        self._fw_set_of = [self._fw_sets.index(names) for names in self.fw_names] or [0] * n_layers

        self._reset_state()
        self.use_fused = True   # fused A->B->C branch kernel when (C, K, L) fits its LDS tile; else 3 stage kernels
        # fused branches on the bf16 matrix cores at fp32 accuracy (spectral_x3.hip: 16 or 8 lines per workgroup -- the library
        # picks 8 while the launch still fits one round of workgroups -- packed pre-split weights) for the axes the library
        # takes (C = 64, K <= 16); 17..32 modes go through the split-bf16 stage kernels
        self.use_x3 = True
        # feed-forward weight gradients of ALL layers as one launch after the backward loop (ffno_ffh_bwd_weights_partial_multi):
        # every layer keeps its own gradient buffer instead of the ping-pong pair; FF_WGRAD_ROUNDS x resident workgroups / L
        # slices per layer
        self.ff_wgrad_deferred = True
        # ... and then the chain kernels leave the sums of their two input tensors unwritten (s_sum / db_sum NULL): every layer keeps
        # both branch outputs and both gradient buffers, the weight-gradient launch adds them while it stages its rows
        #   "s": the forward's input sums (the backward-data launch still writes its summed gradient: leaving that one out too was
        #   measured slower, round 4);  "0": none
        self.ff_lazy_sums = "s"
        self.ff_schedule = 0      # ffno.h FFNO_FF_SCHED_* (0: the library's choice)
        # cap on the persistent workgroups of a feed-forward chain launch (ffno_ff_opts.max_workgroups and the field of the layer
        # descriptors; 0 = one per CU, the library's choice): for callers that share the device with another stream
        self.ff_max_workgroups = 0
        self.x3_min_lines = 1
        # workgroups (= partial slices) of the weight-gradient kernel: one per CU at width 64 (eight waves each), two per CU at
        # width 32 (four waves each: measured 157 -> 165 steps/s at 72^3 x 32 together with three chain workgroups per CU)
        self.ff_wgrad_slices = 512 if width == 32 else 256
        # one C call per layer and direction (ffno_layer_fwd / ffno_layer_bwd: paired branches + feed-forward) instead of two /
        # three; per-kernel timing (a timer attached) needs the individual calls
        self.use_layer_calls = True
        self.infer_self_range = True      # inference layers of axis length <= 64 scale every line from its own maximum (no range words)
        self.infer_stack_any_batch = False      # (see _stack_pays)
        self.infer_min_lines = None      # lines per axis pair from which the inference layer is used (None: more than 4 per CU)
        self.timer = None   # optional KernelTimer (bench.py): HIP-event timing of individual launches
        # fp16x2 packs: max |W| of what goes into them is folded at every n-th rebuild of the derived operands (0 = never) and
        # looked at one rebuild later -- with 1 (the default since round 4: three 3-us launches per step) an overflowing weight
        # is reported after at most one more optimiser step (include/ffno.h: |W| < 65504 is a hard precondition of the packs)
        self.weight_range_check_every = 1
        self._read_environment()

    def _read_environment(self):
        """The switches of INTEGRATION.md, read once here (plain attributes after that)."""
        env = os.environ
        # operand split of the feed-forward kernels: "fp16x2" (ffno_ffh_*: two fp16 planes, three MFMAs per product block,
        # operands range-scaled on the device) or "bf16x3" (ffno_ffx_*: three bf16 planes, six MFMAs, any fp32 range)
        self.ff_split = env.get("FFNO_FF_SPLIT", "fp16x2")
        self.x3_mix_split = env.get("FFNO_X3_MIX_SPLIT", "fp16x2")      # the same for the fused x3 mix and the Fourier-weight gradient
        self.storage = env.get("FFNO_STORAGE", "fp32")      # activations in HBM (include/ffno.h "Storage formats"): "fp32" / "bf16"
        # forward passes that save nothing through the two-launch inference layer (csrc/infer.hip) where it fills the chip ...
        self.use_infer_layer = env.get("FFNO_INFER_LAYER", "1") != "0"
        self.use_infer_stack = env.get("FFNO_INFER_STACK", "1") != "0"      # ... and the whole stack as one persistent launch
        # memory cap of the deferred weight-gradient launch (2 L P C more words with lazy sums, 1.7 GB at the headline shape):
        # beyond it the engine keeps the ping-pong pair and per-layer launches
        self.ff_defer_max_bytes = int(env.get("FFNO_FF_DEFER_MAX_BYTES", 16 << 30))

    def _reset_state(self):
        """Every mutable private attribute, with the value of an engine nothing is bound to yet."""
        self.params: Dict[str, torch.Tensor] = {}
        self.device = None
        self._bind_sig = None       # data pointers of the tensors bind() validated last
        self._issue_stream = None   # torch stream object the next launches go to (None = current stream)
        self._training = False      # the pass in flight draws dropout masks
        self._drop_calls = 0        # training forwards so far: every one draws new masks
        self._in_drop_seed = 0      # seed of the last pass's input-dropout mask (the backward pass regenerates it)
        self._last_plan = None      # the plan of the last forward pass (paired_last, infer_last, _saved_x3, ...)
        self._saved = None          # _Saved of the last forward(save_for_backward=True)
        self.dx = None              # backward(need_dx=True): gradient with respect to the input
        self.forecast_list = []     # use_fork: the per-layer head outputs of the last forward
        self.infer_stack_last = False      # the last forward ran as the persistent inference launch
        self._wr_count = 0          # weight-range check (_check_weight_range): rebuilds counted
        self._wr_warned = False     # ... the small-weight warning was given
        self._reset_device_state()

    def _reset_device_state(self):
        """The part of the state that lives on the device or was derived for it: dropped when the parameters move to another."""
        self._ptr_sig = None        # what _refresh_pointers laid the views, descriptors and packs out for
        self._prep_sig = None       # what _prepare_weights built the derived operands from (None: rebuild)
        self._ws = None             # the current workspace ...
        self._ws_key = None         # ... its key ...
        # ... among the WS_CACHE_MAX used last: train / validation / rollout batches alternate in a real run, full and short, and a
        # multi-resolution run (builders/markov_data.py) switches between grid sizes from one optimiser step to the next
        self._ws_cache = {}
        self._tw: Dict[int, torch.Tensor] = {}      # twiddle tables by axis length
        self._dft_tabs = {}         # DFT-fragment tables by (axis length, modes, direction); False: none for this shape
        self._desc_dev = None       # weight-norm descriptor table ...
        self._n_desc = 0            # ... its rows ...
        self._max_rows = 0          # ... and the longest weight in it
        self._fx_flat = None        # feed-forward operand packs, one buffer ...
        self._fx_dev = None         # ... their descriptor table ...
        self._n_fx = 0              # ... and its rows
        self._fwpack = _lib.CachedTable()      # table of the Fourier-weight pack launch
        self._x3pack = _lib.CachedTable()      # ... of the x3 pack launch
        self._wr_word = None        # weight-range check: the device word ...
        self._wr_late = _DeferredWord(self.device)      # ... the late look at it (max |W|) ...
        self._wr_table = _lib.CachedTable()      # ... and the table of its amax launch

    def _bf16(self) -> bool:
        if self.storage not in ("fp32", "bf16"):
            raise ValueError("storage must be 'fp32' or 'bf16', got %r" % (self.storage,))
        return self.storage == "bf16"

    def _st(self) -> int:
        return 1 if self._bf16() else 0      # FFNO_STORE_F32 / FFNO_STORE_BF16

    def _conc(self) -> bool:
        return bool(self._ffx() and not self.use_fork
                    and self.mode != "no-fourier" and self.spectral == "factorized")

    @staticmethod
    def _schedule(fused, views):
        """(views that run on their own first, (a, b) = the two views that share paired launches | None).
        Preferred: the last two FUSED views (one launch); else the last two STAGED views whose stage kernels share a
        template instance (three paired launches: 256 x 256 with 32 / 64 modes)."""
        n = len(fused)
        fz = [w for w in range(n) if fused[w]]
        sg = [w for w in range(n) if not fused[w]]
        pair = None
        if len(fz) >= 2:
            pair = (fz[-2], fz[-1])
            # a many-mode axis (4-line tiles, the whole weight set streamed per tile) does not share a launch with a <= 16-mode
            # axis: the pair kernel would drag the short axis onto 4-line tiles too (airfoil, 32 x 16 modes: 91 vs 99 steps/s)
            if (views[pair[0]].K > 16) != (views[pair[1]].K > 16):
                pair = None
        elif len(sg) >= 2:
            a, b = sg[-2], sg[-1]
            rt = lambda v: (2 * v.K + 31) // 32      # noqa: E731
            if rt(views[a]) == rt(views[b]) <= 4:
                pair = (a, b)
        if pair is None:
            return list(range(n)), None
        return [w for w in range(n) if w not in pair], pair

    def _pair(self, name, ws, v0, v1, src, dst0, dst1, resid0, save0, save1, planes0, planes1, fwd: bool, st, acc0: int = 0,
              fused: bool = True, x3: bool = False, rin=None, rout=None, resid1=None):
        """Branches of views v0 and v1 side by side -- ONE launch when both are fused, three paired stage launches else:
        dst0 (+)= [resid0 +] branch0(src)  (``acc0``: accumulate into dst0),  dst1 = [resid1 +] branch1(src).
        rin / rout: range words of src / of the two outputs (both branches fold into ``rout``)."""
        lib = _lib.get_lib()
        ck_f, ck_i, conj = (0, 1, 0) if fwd else (1, 0, 1)
        if not fused:
            sv0 = save0 if save0 is not None else ws.SD
            sv1 = save1 if save1 is not None else ws.SD2
            ba = self._branch(v0, src, dst0, resid0, sv0, planes0, acc0, False, fwd, None, rout if x3 else None)
            bb = self._branch(v1, src, dst1, resid1, sv1, planes1, 0, False, fwd, None, rout if x3 else None)
            fn = lib.ffno_spectral_x3_staged_pair if x3 else lib.ffno_spectral_staged_pair      # x3: planes are the packed sets
            self._k("spectral_staged_pair" + ("" if fwd else "(adj)"), fn, ctypes.byref(ba),
                    ctypes.byref(bb), _p(ws.SY), _p(ws.SY2), self.C, ck_f, ck_i, conj, st)
            if not x3:      # the fp32 stage kernels do not fold their output maxima
                self._fold(dst0, rout, st)
                self._fold(dst1, rout, st)
            return
        ba = self._branch(v0, src, dst0, resid0, save0, planes0, acc0, x3, fwd, rin, rout)
        bb = self._branch(v1, src, dst1, resid1, save1, planes1, 0, x3, fwd, rin, rout)
        if x3:       # planes0 / planes1 are the packed split-bf16 sets
            self._k(name, lib.ffno_spectral_x3_pair, ctypes.byref(ba), ctypes.byref(bb), self.C, ck_f, ck_i, conj,
                    X3_INTERLEAVE, st)
            return
        self._k(name, lib.ffno_spectral_fused_pair, ctypes.byref(ba), ctypes.byref(bb), self.C, ck_f, ck_i, conj, st)

    def _branch(self, v, src, dst, resid, save, planes, acc, x3=False, fwd=True, rin=None, rout=None):
        """Branch descriptor; with fp16x2 packs the x3 kernel scales its spectrum tile from the range word of ``src``."""
        fmt = int(v.x3fmt) if (x3 and planes is not None and self._x3_h2()) else 0      # ffno.h FFNO_PLANES_*
        dft = self._dft_frags(v.L, v.K, fwd) if fmt else None
        return _capi.FusedBranch(_p(src), _p(dst), resid, _p(save), _p(planes), _p(self._twiddle(v.L)), v.Bv, v.Mv, v.Nv, v.K,
                                 v.a01, acc, fmt, 0, rin if fmt else None, rout, self._st(), 0, _p(dft))      # (tile_lines 0: library's)

    def _dft_frags(self, L: int, K: int, fwd: bool):
        """DFT-matrix fragment table of the many-mode fused kernel for (axis length, modes, direction): built once per engine and
        device on the launch stream (ffno_spectral_x3_dft_frags), then shared by every line, layer and step."""
        key = (L, K, bool(fwd))
        tab = self._dft_tabs.get(key)
        if tab is None:
            lib = _lib.get_lib()
            nb = int(lib.ffno_spectral_x3_dft_frags_bytes(L, K)) if self.C in (32, 64) else 0      # 0: no table for this shape
            if nb:
                tab = torch.empty(nb // 4, dtype=torch.int32, device=self.device)
                ck_f, ck_i = (0, 1) if fwd else (1, 0)
                self._k("dft_frags", lib.ffno_spectral_x3_dft_frags, _p(self._twiddle(L)), L, K, ck_f, ck_i, _p(tab),
                        _lib.current_stream(self.device))
            else:
                tab = False
            self._dft_tabs[key] = tab
        return tab if tab is not False else None

    # ---- range words (include/ffno.h "Range words"): one uint32 per (tensor kind, layer) in ws.RW ---------------------
    def _ranged(self) -> bool:
        """True when some kernel of this configuration cuts operands into fp16 planes (then every producer on the path
        records its output maximum and every fp16x2 consumer scales from it -- on the device)."""
        return bool((self._ffx() and self._h2()) or (self.use_x3 and self.spectral == "factorized" and self._x3_h2()))

    def _rw(self, ws, kind: str, l: int):
        return ctypes.c_void_p(ws.RW.data_ptr() + 4 * (ws.rw_kinds[kind] * (self.L + 1) + l)) if self._ranged() else None

    def _fw_words(self, ws, l0: int):
        """Range words of the tensors whose spectra the Fourier-weight-gradient launch contracts, from layer l0 on: the layer inputs
        (kind x) and the feed-forward data gradients (kind d) -- (x words, d words) as device pointers, or (None, None): then the
        launch keeps the bf16x3 arithmetic (any range).  fp16x2 (three MFMAs per product instead of six) when the spectral kernels
        run on fp16x2 packs (x3_mix_split), i.e. when every producer on the path records its maximum."""
        if not (self._x3_h2() and self._ranged() and self.spectral == "factorized" and self.use_x3):
            return None, None
        return self._rw(ws, "x", l0), self._rw(ws, "d", l0)

    def _fold(self, t, word, st):
        """Producers that do not record their output maximum themselves: one more pass over the tensor."""
        if word is None or t is None:
            return
        self._k("amax", _lib.get_lib().ffno_amax, _p(t), t.numel(), word, st)

    def _x3_h2(self) -> bool:
        if self.x3_mix_split not in ("fp16x2", "bf16x3"):
            raise ValueError("x3_mix_split must be 'fp16x2' or 'bf16x3', got %r" % (self.x3_mix_split,))
        return self.x3_mix_split == "fp16x2"

    def _ffx(self) -> bool:
        """The feed-forwards run on the split kernels (ffx.hip): whenever they are the fused two-linear shape -- __init__ admits
        only the (width, hidden) pairs of _SUPPORTED_CH, which is those kernels' dispatch set (ffno_ffx_supported)."""
        return not self.general_ff

    def _h2(self) -> bool:
        if self.ff_split not in ("fp16x2", "bf16x3"):
            raise ValueError("ff_split must be 'fp16x2' or 'bf16x3', got %r" % (self.ff_split,))
        return self.ff_split == "fp16x2"

    # ---- the split feed-forward kernels of either family (same operators; own weight packs) ----
    def _ffs_fwd2(self, s, s2, s_sum, resid, l0, b0, b1, out, mask, P, st, rin=None, rout=None):
        lib = _lib.get_lib()
        fn = lib.ffno_ffh_fwd2 if self._h2() else lib.ffno_ffx_fwd2
        o = _capi.FfOpts(rin, rout, int(self.ff_max_workgroups), int(self.ff_schedule), self._st())
        self._k("ff_fwd", fn, _p(s), _p(s2), _p(s_sum), _p(resid), _p(l0.fx[0]), _p(b0), _p(l0.fx[1]), _p(b1), _p(out), _p(mask),
                P, self.C, self.H, ctypes.byref(o), st)

    def _ffs_bwd2(self, g, g2, g_sum, mask, l0, ds, P, st, rin=None, rout=None):
        lib = _lib.get_lib()
        fn = lib.ffno_ffh_bwd_data2 if self._h2() else lib.ffno_ffx_bwd_data2
        o = _capi.FfOpts(rin, rout, int(self.ff_max_workgroups), int(self.ff_schedule), self._st())
        self._k("ff_bwd_data", fn, _p(g), _p(g2), _p(g_sum), _p(mask), _p(l0.fx[2]), _p(l0.fx[3]), _p(ds),
                P, self.C, self.H, ctypes.byref(o), st)

    def _ffs_wgrad(self, s, g, l0, b0, part, P, nsplit, st, rs=None, rg=None):
        lib = _lib.get_lib()
        args = (_p(s), _p(g), _p(l0.fx[0]), _p(b0), _p(l0.fx[2]), _p(part), P, self.C, self.H, nsplit)
        if self._h2():
            self._k("ff_bwd_weights_partial", lib.ffno_ffh_bwd_weights_partial, *args, rs, rg, self._st(), st)
        else:
            self._k("ff_bwd_weights_partial", lib.ffno_ffx_bwd_weights_partial, *args, st)

    # ------------------------------------------------------------------------------------------------
    def bind(self, params: Dict[str, torch.Tensor]):
        """Attach the parameter tensors (unique reference names -> fp32 contiguous device tensors)."""
        # the same storage as last time (a module re-binds its detached parameters on every forward): validated already
        sig = tuple(params[n].data_ptr() for n in self.param_names) if all(n in params for n in self.param_names) else None
        if sig is not None and self.params and sig == self._bind_sig:
            self.params = {n: params[n] for n in self.param_names}
            return
        dev = self._validate(params)
        self.params = {n: params[n] for n in self.param_names}
        self._bind_sig = sig
        if dev != self.device:
            self.device = dev
            self._alloc_param_buffers()
        self._ptr_sig = None

    def _alloc_param_buffers(self):
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.gflat = torch.zeros(self.n_params, **f32)
        n_eff = sum(l.rows * l.cols for l in self.linears.values()) if self.wnorm else 0
        self.weff_flat = torch.empty(max(n_eff, 1), **f32)
        self.gweff_flat = torch.zeros(max(n_eff, 1), **f32)
        self.fold = torch.zeros(self.O * (self.C + 1), **f32)
        # mode-major weight planes: planes[set][w] = (wp, wpt), each 2*K_w*C*C floats
        plane_modes = [2 * self.K * self.K] if self.spectral == "plus" else list(self.Ks)   # plus: one joint (ky, kx') set
        self.planes = [[(torch.empty(2 * K * self.C * self.C, **f32), torch.empty(2 * K * self.C * self.C, **f32))
                        for K in plane_modes] for _ in range(max(len(self._fw_sets), 1))]
        # packed split-bf16 twins of the planes for the x3 branch kernel: xplanes[set][w] = (forward, adjoint) or None
        lib = _lib.get_lib()
        self.xplanes = [[None] * len(plane_modes) for _ in self.planes]
        if self.spectral == "factorized" and self.mode == "full":
            for si in range(len(self.planes)):
                for w, K in enumerate(plane_modes):
                    nb = int(lib.ffno_spectral_x3_pack_bytes(self.C, K))      # 0 = no split kernel for (C, K)
                    if nb:
                        self.xplanes[si][w] = tuple(torch.empty(nb // 4, dtype=torch.int32, device=dev) for _ in range(2))
        self._reset_device_state()

    def _refresh_pointers(self):
        sig = tuple(self.params[n].data_ptr() for n in self.param_names) + (self.ff_split,)
        if sig == self._ptr_sig:
            return
        self._ptr_sig = sig
        off = 0
        descs = []
        for lin in self.linears.values():
            n = lin.rows * lin.cols
            if lin.wnorm:
                lin.weff = self.weff_flat[off:off + n].view(lin.rows, lin.cols)
                lin.gweff = self.gweff_flat[off:off + n].view(lin.rows, lin.cols)
                off += n
                g, v = self.params[lin.prefix + "weight_g"], self.params[lin.prefix + "weight_v"]
                descs.append(_capi.WnDesc(g.data_ptr(), v.data_ptr(), lin.weff.data_ptr(), lin.gweff.data_ptr(),
                                          self.grad_view(lin.prefix + "weight_g").data_ptr(),
                                          self.grad_view(lin.prefix + "weight_v").data_ptr(), lin.rows, lin.cols))
            else:
                lin.weff = self.params[lin.prefix + "weight"]
                lin.gweff = self.grad_view(lin.prefix + "weight")
        self._n_desc = len(descs)
        # split-bf16 operand packs of every feed-forward block (include/ffno.h "packed"): forward A1/A2, backward A1/A2
        lib = _lib.get_lib()
        blocks = list(dict.fromkeys(self.ff_prefix + self.fc_prefix))
        if self._ffx():
            words = int((lib.ffno_ffh_pack_bytes if self._h2() else lib.ffno_ffx_pack_bytes)(self.C, self.H)) // 4
            if self._fx_flat is None or self._fx_flat.numel() != 4 * words * len(blocks):
                self._fx_flat = torch.empty(4 * words * len(blocks), dtype=torch.int32, device=self.device)
            fdescs = []
            for bi, pfx in enumerate(blocks):
                l0, l1 = self.linears[pfx + "layers.0.0."], self.linears[pfx + "layers.1.0."]
                pk = [self._fx_flat[(4 * bi + q) * words:(4 * bi + q + 1) * words] for q in range(4)]
                l0.fx = pk      # both linears of the block see the four packs
                l1.fx = pk
                C_, H_ = self.C, self.H
                for (src, sh, sc, ty), dst in zip(((l0.weff, C_, 1, 1), (l1.weff, 1, H_, 2), (l1.weff, 1, H_, 1),
                                                   (l0.weff, C_, 1, 2)), pk):
                    fdescs.append(_capi.FxPackDesc(src.data_ptr(), dst.data_ptr(), sh, sc, ty, 0))
            self._n_fx = len(fdescs)
            self._fx_dev = _lib.device_table(_capi.FxPackDesc, fdescs, self.device)
        self._max_rows = max([l.rows for l in self.linears.values()])
        self._desc_dev = _lib.device_table(_capi.WnDesc, descs, self.device) if descs else None

    def _twiddle(self, L: int) -> torch.Tensor:
        tw = self._tw.get(L)       # (this engine's memo of the package's one table cache: asked once per branch launch)
        if tw is None:
            tw = self._tw[L] = _lib.twiddle(L, self.device)
        return tw

    # ------------------------------------------------------------------------------------------------
    def _views(self, B: int, Sp: Sequence[int]) -> List[_View]:
        """views[w] = the axis mixed by fourier_weight[w], as a [Bv, Mv, Nv, C] view of the (padded) buffer."""
        C = self.C
        if self.spectral == "plus":
            # one joint (ky, kx') mode set: the chain (ws.chain) stands in for the view (rows per mode = samples, spec = 2-D spectrum)
            return [CornerChain(B, Sp, (self.K, self.K), C, lambda *a: self._k(*a), self.device)]
        if self.nd == 2:
            M, N = Sp
            if self.first_axis_first:      # mesh_2d.py:71-75,92-96: weight 0 <-> x (first axis), weight 1 <-> y (last axis)
                return [_View(B, M, N, 1, self.Ks[0], C), _View(B, M, N, 0, self.Ks[1], C)]
            return [_View(B, M, N, 0, self.Ks[0], C), _View(B, M, N, 1, self.Ks[1], C)]
        X, Y, Z = Sp
        return [_View(B, X, Y * Z, 1, self.Ks[0], C),       # x: lines (b, y, z), stride Y*Z*C
                _View(B * X, Y, Z, 1, self.Ks[1], C),       # y: lines (b, x, z), stride Z*C
                _View(B, X * Y, Z, 0, self.Ks[2], C)]       # z: contiguous lines (b, x, y)

    def _workspace_key(self, B: int, S: Tuple[int, ...], save: bool):
        """The geometry and everything a workspace's buffers and schedule decisions (deferred weight-gradient launch, lazy input
        sums, slice counts) are derived from: an attribute switched on a live engine gets a workspace laid out for it instead of
        decisions frozen for the old value."""
        return (B, tuple(S), bool(save), self._ffx(), self._conc(), self.general_ff, self._bf16(),
                (self._h2(), self._ranged(), bool(self.ff_wgrad_deferred), str(self.ff_lazy_sums), int(self.ff_wgrad_slices),
                 bool(self.use_x3), bool(self.use_fused), int(self.ff_defer_max_bytes)))

    def _workspace(self, B: int, S: Tuple[int, ...], save: bool):
        key = self._workspace_key(B, S, save)
        if self._ws_key == key:
            return self._ws
        cache = self._ws_cache
        if key in cache:      # (no re-allocation)
            self._ws, self._ws_key = cache.pop(key), key
            cache[key] = self._ws      # most recently used last: eviction below takes the one unused for longest
            return self._ws
        lib = _lib.get_lib()
        dev, C, H, L, O = self.device, self.C, self.H, self.L, self.O
        Sp = tuple(s + self.pad for s in S)
        P_in = B * int(np.prod(S))            # unpadded pixels (inputs / outputs)
        P = B * int(np.prod(Sp))              # pixels of the activation buffers
        f32 = dict(dtype=torch.float32, device=dev)
        act = dict(dtype=torch.bfloat16 if self._bf16() else torch.float32, device=dev)     # activation tensors of the layer stack
        ns = L if save else 1
        ws = _Workspace()
        ws.P, ws.P_in, ws.Sp = P, P_in, Sp
        ws.views = self._views(B, Sp)
        if self.pad:
            s3 = (1,) * (3 - self.nd) + tuple(S)
            p3 = (1,) * (3 - self.nd) + tuple(Sp)
            ws.padmap = _capi.PadMap((ctypes.c_int32 * 3)(*s3), (ctypes.c_int32 * 3)(*p3))
            ws.pm = ctypes.byref(ws.padmap)
        ws.X = torch.empty(P, C, **act)
        ws.Blast = torch.empty(P, C, **act)
        ws.Y = torch.empty(P_in * O, **f32)
        ws.S = torch.empty(ns, P, C, **act)
        nv = len(ws.views)
        ws.SXall = [torch.empty(ns, v.spec, **f32) for v in ws.views]
        ws.SY = torch.empty(max(v.spec for v in ws.views), **f32)
        ws.SD = torch.empty(max(v.spec for v in ws.views), **f32)
        if self._conc():
            ws.SD2 = torch.empty_like(ws.SD)
            ws.SY2 = torch.empty_like(ws.SY)
            ws.T = torch.empty(P, C, **act)
            if save:
                ws.G1 = torch.empty(P, C, **act)
        if self.spectral == "plus":
            ws.chain = ws.views[0]
            ws.scr = ws.chain.scratch(lambda n: torch.empty(n, **f32))
        ws.mask_words = int(lib.ffno_ff_mask_words(P, H))
        ws.rw_kinds = {"x": 0, "s": 1, "g": 2, "d": 3, "t": 4, "f": 5}
        ws.RW = torch.zeros(len(ws.rw_kinds) * (L + 1), dtype=torch.int32, device=dev)
        if self.layer_norm:
            ws.TL = torch.empty(ns, P, C, **f32)
            ws.LNS = torch.empty(ns, P, 2, **f32)
            if self.use_fork:
                ws.TLF = torch.empty(ns, P, C, **f32)
                ws.LNSF = torch.empty(ns, P, 2, **f32)
            if save:
                ws.DT = torch.empty(P, C, **f32)
                ws.lnpart = torch.empty(2 * C * int(lib.ffno_layernorm_nsplit(P)), **f32)
                if self.use_fork:
                    ws.DTF = torch.empty(P, C, **f32)
        if self.use_fork:
            ws.F = torch.empty(ns, P, C, **f32)
            ws.YL = torch.empty(L, P_in * O, **f32)
        if self.general_ff:
            kinds = ["backcast"] + (["forecast"] if self.use_fork else [])
            ws.HG = {kind: [[torch.empty(P, H, **f32) for _ in range(self.n_ff - 1)] for _ in range(ns)] for kind in kinds}
            if save:
                ws.DA = [torch.empty(P, H, **f32) for _ in range(2)]
                ws.glpart = torch.empty(int(lib.ffno_glin_wgrad_partial_floats(P, H, H)), **f32)
        if save and self.use_fork:
            ws.MASKF = torch.zeros(ns, ws.mask_words, dtype=torch.int32, device=dev)
            ws.DSF = torch.empty(P, C, **f32)
            ws.GF = torch.empty(P, C, **f32)
            ws.redl = torch.empty(O * (C + 1), **f32)
        if save:
            ws.MASK = torch.zeros(ns, ws.mask_words, dtype=torch.int32, device=dev)
            ws.DS = torch.empty(P, C, **act)
            ws.defer_wgrad = bool(self.ff_wgrad_deferred and self._ffx() and self._h2() and self._ranged() and not self.share_fork
                                  and self._plain_layer and (C, H) in ((64, 256), (32, 128)) and self.mode != "no-fourier")
            if 2 * L * P * C * (2 if self._bf16() else 4) > int(self.ff_defer_max_bytes):      # (its memory cost)
                ws.defer_wgrad = False
            ws.G = [torch.empty(P, C, **act) for _ in range(L + 1 if ws.defer_wgrad else 2)]
            if self.ff_lazy_sums not in ("s", "0", ""):
                raise ValueError("ff_lazy_sums must be 's' or '0', got %r" % (self.ff_lazy_sums,))
            ws.lazy_sums = "s" if (ws.defer_wgrad and self.ff_lazy_sums == "s" and self._conc() and (C, H) == (64, 256)) else ""
            if ws.lazy_sums:
                ws.TS = [torch.empty(P, C, **act) for _ in range(L)]
            ws.SDall = [torch.empty(L, v.spec, **f32) for v in ws.views] if self.mode == "full" else None
            ws.nsplit_ff = max(1, min(int(self.ff_wgrad_slices), (P + 127) // 128))
            cus = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else 256
            ws.nsplit_ffm = max(1, min(ws.nsplit_ff, (FF_WGRAD_ROUNDS * (3 if H <= 128 else 1) * cus) // L))
            ws.wg_table = _lib.CachedTable()
            ws.ffpart = torch.empty(int(lib.ffno_ff_wgrad_partial_floats(C, H, ws.nsplit_ff)), **f32)
            ws.defer_reduce = bool(self._ffx() and not self.share_fork)
            if ws.defer_reduce:
                njobs = L * (2 if self.use_fork else 1)
                ws.ffparts = torch.empty(njobs, ws.ffpart.numel(), **f32)
                ws.red_table = _lib.CachedTable()
            ws.nsplit_fw = [max(1, min(max(1, FW_GRAD_WGS // v.K), (L * v.R + 63) // 64)) for v in ws.views]
            if self.spectral == "plus":
                ws.nsplit_fw = [1]
            ws.fwpart = [[torch.empty(ws.nsplit_fw[w] * 2 * ws.views[w].modes * C * C, **f32) for w in range(nv)]
                         for _ in range(max(len(self._fw_sets), 1))]
            ws.fwpart_multi, ws.fwgrad_tab, ws.fwgrad_sig = [None] * nv, [None] * nv, [None] * nv
            ws.nsplit_lift = max(1, min(1024, (P_in + 127) // 128))     # all slices co-resident (16 KB LDS per workgroup)
            ws.liftpart = torch.empty(ws.nsplit_lift * C * (self.Cin + 1), **f32)
            ws.nsplit_head = max(1, min(256, (P_in + 255) // 256))
            ws.headpart = torch.empty(ws.nsplit_head * O * (C + 1), **f32)
            ws.red = torch.empty(O * (C + 1), **f32)
        self._ws, self._ws_key = ws, key
        cache[key] = ws
        while len(cache) > WS_CACHE_MAX:
            cache.pop(next(iter(cache)))
        return ws

    def _saved_pass(self, what: str = "backward()") -> _Saved:
        """What the last ``forward(save_for_backward=True)`` saved, the workspace it filled included.  A schedule / arithmetic
        attribute switched since then (``ff_split``, ``x3_mix_split``, ``ff_wgrad_deferred``, ``ff_lazy_sums``, ``use_x3``,
        ``use_fused``, ``storage``, slice counts) would select ANOTHER workspace -- and the kernels of this pass read some of them
        as they are now: refuse instead of differentiating uninitialised memory."""
        sv = self._saved
        if sv is None:
            raise RuntimeError(f"{what} needs a preceding forward(save_for_backward=True)")
        if self._workspace_key(sv.B, sv.S, True) != sv.ws_key:
            raise RuntimeError("an engine attribute that shapes the workspace (ff_split / x3_mix_split / ff_wgrad_deferred / "
                               "ff_lazy_sums / ff_wgrad_slices / use_x3 / use_fused / storage) changed between forward() and "
                               "backward(): run the forward pass again")
        return sv

    def weights_changed(self):
        """Tell the engine that parameter memory was written behind PyTorch's back (a raw-pointer kernel such as the fused
        AdamW of FFNOTrainer): the derived operands (weight-norm products, packed fragments, folded head) are rebuilt by the
        next forward.  In-place torch ops on the BOUND tensors or on anything that shares their version counter (the module
        mirrors and FFNOTrainer bind ``parameter.detach()``: optimizer.step(), load_state_dict, p.copy_() are seen) need no
        call; writes through another alias of the same memory (a view of a flat buffer, ``p.data``'s source) do."""
        self._prep_sig = None

    def _prepare_weights(self, st, x3fmt: List[int]):
        lib = _lib.get_lib()
        self._refresh_pointers()
        # derived operands only depend on the parameters and the arithmetic choices: an inference loop (rollout: 10-100 forwards
        # on the same weights) prepares them once -- five launches less per forward
        try:
            sig = (tuple((t.data_ptr(), t._version) for t in self.params.values()), self.ff_split, self.x3_mix_split,
                   tuple(x3fmt), self.use_x3, getattr(st, "value", st))
        except RuntimeError:      # inference tensors (created under torch.inference_mode()) have no version counter:
            sig = None            # nothing to compare -- the operands are rebuilt by every forward, as before round 3
        if sig is not None and sig == self._prep_sig:
            return
        self._prep_sig = sig
        if self._desc_dev is not None:
            self._k("weightnorm_fwd", lib.ffno_weightnorm_fwd, _p(self._desc_dev), self._n_desc, self._max_rows, st)
        if self._ffx() and self._n_fx:
            self._k("ffx_pack", lib.ffno_ffh_pack if self._h2() else lib.ffno_ffx_pack, _p(self._fx_dev), self._n_fx, self.C,
                    self.H, st)
        for i, names in enumerate(self._fw_sets if self.spectral == "plus" else []):
            self._k("fw2d_pack", lib.ffno_fw2d_pack, _p(self.params[names[0]]), _p(self.params[names[1]]),
                    _p(self.planes[i][0][0]), _p(self.planes[i][0][1]), self.C, self.K, st)
        if self.spectral != "plus" and self._fw_sets:      # every (weight set, axis) tensor in ONE launch
            rows = tuple((self.params[n].data_ptr(), self.planes[i][w][0].data_ptr(), self.planes[i][w][1].data_ptr(), self.Ks[w],
                          int(self.spectral == "dct")) for i, names in enumerate(self._fw_sets) for w, n in enumerate(names))
            self._k("fw_pack", lib.ffno_fw_pack_batched, _p(self._fwpack.get(_capi.FwPackDesc, rows, self.device)), len(rows),
                    self.C, max(self.Ks), st)
            if self.use_x3 and any(x is not None for row in self.xplanes for x in row):
                rows = tuple((self.planes[i][w][d].data_ptr(), xp[d].data_ptr(), self.Ks[w], x3fmt[w])
                             for i, row in enumerate(self.xplanes) for w, xp in enumerate(row) if xp is not None for d in range(2))
                self._k("fw_pack_x3", lib.ffno_spectral_x3_pack, _p(self._x3pack.get(_capi.X3PackDesc, rows, self.device)),
                        len(rows), self.C, max(r[2] for r in rows), st)
        o0, o1 = self.linears["out.0."], self.linears["out.1."]
        self._k("head_fold", lib.ffno_head_fold, _p(o0.weff), _p(self.params["out.0.bias"]), _p(o1.weff),
                _p(self.params["out.1.bias"]), _p(self.fold), self.C, HEAD_DIM, self.O, st)
        self._check_weight_range(st, x3fmt)

    # ---- the one operand the range words do not cover: the WEIGHTS inside the fp16x2 packs ---------------------------------
    def _check_weight_range(self, st, x3fmt: List[int]):
        """Activations, spectra and gradients are brought into the half format's range per launch (range words).  Weights are
        packed as they are: one at or above 65504 would overflow its fp16 planes.  Every ``weight_range_check_every``-th time
        the derived operands are rebuilt, max |W| of everything that goes into an fp16x2 pack is folded on the device
        (ffno_amax) and copied to pinned host memory asynchronously; the value is looked at the next time round -- no
        synchronisation, the error arrives a few steps late but it arrives (the loss is NaN by then, and says why)."""
        every = int(self.weight_range_check_every)
        fp16_ff, fp16_mix = self._ffx() and self._h2(), any(x3fmt)
        if every <= 0 or not (fp16_ff or fp16_mix):
            return
        host = self._wr_late.take()
        if host is not None:
            wmax = float(host.view(torch.float32)[0])
            if 0.0 < wmax < 2.0 ** -9 and not self._wr_warned:
                import warnings
                self._wr_warned = True
                warnings.warn(f"every weight that goes into the split-fp16 packs is below {wmax:.3g}: the packs keep a fixed "
                              f"absolute error of 2^-36 there, i.e. relative accuracy degrades as the weights shrink "
                              f"(1e-6 at 2e-5); ff_split / x3_mix_split = 'bf16x3' is exact at any magnitude", RuntimeWarning)
            if not wmax < 65504.0:
                raise FloatingPointError(
                    f"a weight of magnitude {wmax:.3g} does not fit the split-fp16 packs (|W| < 65504): set "
                    f"engine.ff_split = engine.x3_mix_split = 'bf16x3' (FFNO_FF_SPLIT / FFNO_X3_MIX_SPLIT) -- any fp32 range")
        self._wr_count += 1
        if (self._wr_count - 1) % every or self._wr_late.pending:
            return
        lib = _lib.get_lib()
        if self._wr_word is None:
            self._wr_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._wr_word.zero_()
        srcs = []
        if fp16_ff:
            if self.wnorm:
                srcs.append(self.weff_flat)       # every effective linear weight, one buffer
            else:
                srcs += [self.params[p + "weight"] for p in self.linears if "_ff." in p and p + "weight" in self.params]
        if fp16_mix:
            srcs += [self.params[n] for names in self._fw_sets for n in names]
        # ONE launch for all of them (per-layer Fourier weights are 2-3 tensors per layer: the airfoil model issued 49 of these
        # 4-us launches per step until round 5); the descriptor table is rebuilt when a tensor moved
        rows = tuple((t.data_ptr(), t.numel()) for t in srcs)
        self._k("amax", lib.ffno_amax_batched, _p(self._wr_table.get(_capi.AmaxDesc, rows, self.device)), len(rows),
                max(n for _, n in rows), _p(self._wr_word), st)
        self._wr_late.post(self._wr_word)

    def _ff_weights(self, l, prefixes=None):
        """(linear 0, linear 1, bias 0, bias 1) of layer l's backcast (or, prefixes = fc_prefix, forecast) feed-forward."""
        fp = (prefixes or self.ff_prefix)[l]
        l0, l1 = self.linears[fp + "layers.0.0."], self.linears[fp + "layers.1.0."]
        return l0, l1, self.params[fp + "layers.0.0.bias"], self.params[fp + "layers.1.0.bias"]

    def _ff_bwd_weights(self, ws, s, s2, g, l0, l1, b0, gb0, gb1, accumulate, P, st, rs=None, rg=None):
        """Weight gradients of one two-linear feed-forward block (``s2``: second addend of s with lazy input sums, else None)."""
        lib = _lib.get_lib()
        if ws.defer_reduce:
            assert not accumulate
            part = ws.ffparts[len(ws.red_jobs)]
            if ws.wg_jobs is not None:
                ws.wg_jobs.append((s.data_ptr(), g.data_ptr(), l0.fx[0].data_ptr(), b0.data_ptr(), l0.fx[2].data_ptr(),
                                   part.data_ptr(), rs.value, rg.value, s2.data_ptr() if s2 is not None else 0, 0))
            else:
                self._ffs_wgrad(s, g, l0, b0, part, P, ws.nsplit_ff, st, rs, rg)
            ws.red_jobs.append((part.data_ptr(), l0.gweff.data_ptr(), l1.gweff.data_ptr(), gb0.data_ptr(), gb1.data_ptr()))
        else:
            self._ffs_wgrad(s, g, l0, b0, ws.ffpart, P, ws.nsplit_ff, st, rs, rg)
            self._k("ff_bwd_weights_reduce", lib.ffno_ffx_bwd_weights_reduce, _p(ws.ffpart), _p(l0.gweff), _p(l1.gweff),
                    _p(gb0), _p(gb1), self.C, self.H, ws.nsplit_ff, accumulate, st)

    # ---- the GENERAL feed-forward path (n_ff_layers != 2 or dropout > 0): one glin kernel per linear layer ------------------
    def _drop_args(self, layer: int, kind: str, k: int):
        """(p, seed) of the dropout site behind linear k of a feed-forward block in this pass: a new mask per training forward,
        layer, block kind and site; the backward pass regenerates it from the same pair."""
        if not (self.dropout > 0.0 and self._training):
            return 0.0, 0
        return self.dropout, _site_seed(self.drop_seed, self._drop_calls, layer, k + 1, int(kind == "forecast"))

    def _ffg_fwd(self, ws, prefix, kind, layer, sv, s, resid, out, P, st, rout=None):
        lib = _lib.get_lib()
        a = s
        for k in range(self.n_ff):
            last = k == self.n_ff - 1
            lin = self.linears[prefix + f"layers.{k}.0."]
            dst = out if last else ws.HG[kind][sv][k]
            p, seed = self._drop_args(layer, kind, k)
            self._k("ff_fwd", lib.ffno_glin_fwd, _p(a), _p(lin.weff), _p(self.params[prefix + f"layers.{k}.0.bias"]),
                    _p(resid) if last else None, _p(dst), P, lin.cols, lin.rows, int(not last), p, seed, st)
            a = dst
        self._fold(out, rout, st)

    def _ffg_bwd(self, ws, prefix, kind, layer, s, g, ds, accumulate, P, st, rout=None):
        """g = dL/d(feed-forward output) -> ds = dL/ds, and the parameter gradients of every linear of the block."""
        lib = _lib.get_lib()
        gv = self.grad_view
        g_cur = g
        for k in reversed(range(self.n_ff)):
            last = k == self.n_ff - 1
            lin = self.linears[prefix + f"layers.{k}.0."]
            x_in = s if k == 0 else ws.HG[kind][layer][k - 1]
            y = None if last else ws.HG[kind][layer][k]
            p, seed = self._drop_args(layer, kind, k)
            self._k("ff_bwd_weights_partial", lib.ffno_glin_bwd_weights, _p(g_cur), _p(y), _p(x_in), _p(ws.glpart), _p(lin.gweff),
                    _p(gv(prefix + f"layers.{k}.0.bias")), P, lin.cols, lin.rows, p, seed, int(accumulate), st)
            dx = ds if k == 0 else ws.DA[k & 1]
            self._k("ff_bwd_data", lib.ffno_glin_bwd_data, _p(g_cur), _p(y), _p(lin.weff), _p(dx), P, lin.cols, lin.rows, p, seed,
                    0, st)
            g_cur = dx
        self._fold(ds, rout, st)

    def _planes_for(self, si, w, adj: int, x3: bool):
        if self.mode != "full":
            return None
        return self.xplanes[si][w][adj] if x3 else self.planes[si][w][adj]

    def _can_fuse(self, views):
        """Per axis: the fused branch kernel when its LDS tile holds (C, K_axis, L_axis), else the three stage kernels
        (e.g. plasticity: x with 32 modes is staged, y / z with 12 / 8 modes are fused)."""
        lib = _lib.get_lib()
        if self.spectral == "plus":
            return [False]
        if self.spectral == "dct":
            return [False] * len(views)
        # fused = the fp32-MFMA fused kernel takes the shape, or the split (x3) fused kernels do (K <= 16 on the 16-line tile,
        # 17..64 modes on the 4-line tile of spectral_x3k: 256 x 256 grids)
        return [bool(self.use_fused and self.mode != "no-fourier"
                     and (lib.ffno_spectral_fused_supported(self.C, v.K, v.L) or self._x3_ok(w, v, views)))
                for w, v in enumerate(views)]

    def _x3_ok(self, w, v, views) -> bool:
        lib = _lib.get_lib()
        if not (self.use_x3 and self.spectral == "factorized" and self.mode != "no-fourier"):
            return False
        P4 = 4 * self.C * max(u.Bv * u.Mv * u.Nv for u in views)       # 32-bit byte offsets inside the kernel
        return bool(v.R >= self.x3_min_lines and P4 < 2 ** 32 and lib.ffno_spectral_x3_supported(self.C, v.K, v.L)
                    and (self.mode != "full" or self.xplanes[0][w] is not None))

    def _infer_ok(self, ws, conc, pair, singles, x3pair, fused) -> bool:
        """The two-launch inference layer (ffno_layer_infer) serves this forward: both axes of a 2-D layer in one paired launch of
        the fused split kernels with fp16x2 packs and <= 16 modes, width 64 / hidden 256 on the split-fp16 feed-forward, fp32
        activations, no fork heads / LayerNorm / dropout -- and enough lines to fill the chip."""
        if not (self.use_infer_layer and conc and pair is not None and not singles and x3pair and fused[pair[0]]):
            return False
        if not (self.nd == 2 and self.mode == "full" and self.spectral == "factorized" and self._ffx() and self._h2() and self._x3_h2()
                and not self._bf16() and self._plain_layer and (self.C, self.H) == (64, 256)):
            return False
        va, vb = ws.views[pair[0]], ws.views[pair[1]]
        if {va.a01, vb.a01} != {0, 1} or (va.Bv, va.Mv, va.Nv) != (vb.Bv, vb.Mv, vb.Nv):
            return False
        if any(v.x3fmt != 1 for v in (va, vb)):
            return False
        row, col = (va, vb) if va.a01 == 0 else (vb, va)
        lib = _lib.get_lib()
        if not lib.ffno_layer_infer_supported(va.Bv, va.Mv, va.Nv, self.C, self.H, row.K, col.K):
            return False
        if self._dft_frags(row.L, row.K, True) is None or self._dft_frags(col.L, col.K, True) is None:
            return False
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count if self.device.type == "cuda" else 256
        need = self.infer_min_lines if self.infer_min_lines is not None else 4 * cus + 1
        return va.R + vb.R >= need

    def _stack_pays(self, B: int) -> bool:
        """The persistent launch runs CUs / 8 = 32 groups of 8 workgroups (16 groups of 16 for a batch <= 16), a group per image: a
        batch below the group count leaves groups idle, a larger one makes groups walk images in rounds of 32.  Measured against the
        per-layer launches (`tools/ab_stack_batch.py`, `profiles/r06_stack_batch.log`; their own row-tile rule was fixed at the end of the
        round, which is what these figures are against): -3 ... -6 % at 9 / 12 / 16 / 24 images, -9 % at 19, -2 ... -6 % at 32 / 48 / 64 /
        96, but +5 % at 40 (a last round with a quarter of the groups busy): a last round of 1..16 images keeps the per-layer launches.
        `engine.infer_stack_any_batch = True` takes it regardless."""
        if self.infer_stack_any_batch:
            return True
        if B <= 16:      # (16 members per image: 8-line / 4-row tiles, 0.98-1.00 ms per forward at 9 / 12 / 16 images against 1.01-1.06)
            return True
        tail = B % 32
        return tail == 0 or tail > 16

    def _run_infer_stack(self, ws, pair, st) -> bool:
        """Enqueue ffno_infer_stack over ws.X (in place; the last layer's feed-forward output lands in ws.Blast).  False: not this
        shape / device, or the persistent launch reported a placement or barrier error (then it is switched off for this engine and
        the caller runs the per-layer launches)."""
        lib = _lib.get_lib()
        C, H, L = self.C, self.H, self.L
        a, b = pair
        va, vb = ws.views[a], ws.views[b]
        row, col = (va, vb) if va.a01 == 0 else (vb, va)
        if int(lib.ffno_infer_stack_supported(va.Bv, va.Mv, va.Nv, C, H, row.K, col.K, L)) != 2:
            return False
        if not self._stack_pays(va.Bv):
            return False
        if ws.stack_sync is None:
            n = int(lib.ffno_infer_stack_sync_words(va.Bv))
            ws.stack_sync = torch.zeros(n, dtype=torch.int32, device=self.device)
            ws.stack_late = _DeferredWord(self.device)
        host = ws.stack_late.take()      # the error word of a PREVIOUS persistent launch on this workspace (copied without synchronising)
        if host is not None and int(host[0]) != 0:
            self.use_infer_stack = False
            raise RuntimeError("ffno_infer_stack: the previous forward pass reported a workgroup without a group or a barrier "
                               "time-out (error word %d): its result was invalid; the persistent launch is now off for this "
                               "engine (engine.use_infer_stack)" % int(host[0]))
        ba = self._branch(va, ws.X, ws.MIX[0], None, None, None, 0, True, True, None, None)
        bb = self._branch(vb, ws.X, ws.MIX[1], None, None, None, 0, True, True, None, None)
        for br, v in ((ba, va), (bb, vb)):
            br.planes_format, br.flags, br.in_amax = 1, _capi.BRANCH_SELF_RANGE, None
            br.dft_frags = _p(self._dft_frags(v.L, v.K, True))
        rows = []
        for l in range(L):
            si = self._fw_set_of[l]
            l0, l1, b0, b1 = self._ff_weights(l)
            rows.append(_capi.InferStackLayer(_p(self._planes_for(si, a, 0, True)), _p(self._planes_for(si, b, 0, True)), _p(l0.fx[0]),
                                              _p(b0), _p(l0.fx[1]), _p(b1)))
        arr = (_capi.InferStackLayer * L)(*rows)
        d = _capi.InferStackDesc(ba, bb, ctypes.cast(arr, ctypes.c_void_p), L, C, H, 0, _p(ws.Blast), _p(ws.stack_sync))
        rc = self._timed("infer_stack", lib.ffno_infer_stack, ctypes.byref(d), st)      # (bench.py: HIP events around it)
        if rc != 0:      # (e.g. the persistent launch was refused: the kernel does not fit once per CU on this device)
            self.use_infer_stack = False
            return False
        err_word = ws.stack_sync[-1:]
        ws.stack_calls += 1
        if not ws.stack_checked:
            # first persistent launch on this workspace: look at its error word before trusting the path
            ws.stack_checked = True
            if int(err_word.cpu()[0]) != 0:
                self.use_infer_stack = False
                import warnings
                warnings.warn("ffno_infer_stack reported a placement / barrier error on this device: using the per-layer launches",
                              RuntimeWarning)
                raise _StackRetry()
        elif self.device.type == "cuda" and not ws.stack_late.pending and ws.stack_calls % 16 == 0:
            # (every 16th launch: the 4-byte copy is a launch of its own; an error after the first checked launch would be a
            #  hardware / scheduling anomaly -- it is reported a few passes late, but it is reported)
            ws.stack_late.post(err_word)
        return True

    def _spectral(self, name, ws, v: _View, src, dst, resid, save, planes, fwd: bool, accumulate: int, fused: bool, st,
                  x3: bool = False, rin=None, rout=None):
        """One spectral branch  dst (+)= [resid +] iDFT(mix(DFT(src)))  along view v (forward or adjoint);
        rin / rout = range words of src / dst."""
        lib, C = _lib.get_lib(), self.C
        ck_f, ck_i, conj = (0, 1, 0) if fwd else (1, 0, 1)
        if fused and x3:
            br = self._branch(v, src, dst, resid, save, planes, accumulate, True, fwd, rin, rout)
            self._k(name, lib.ffno_spectral_x3, ctypes.byref(br), C, ck_f, ck_i, conj, st)
            return
        if self.spectral == "plus":         # (v is ws.chain: the operator's one "view" is the corner chain)
            ws.chain.conv(src, dst, save if save is not None else ws.SD, ws.SY, planes, ws.scr, fwd, st, resid, accumulate)
        elif self.spectral == "dct":       # DCT branch: the same transform pair serves the forward and the adjoint (orthonormal)
            spec = save if save is not None else ws.SD
            self._k("dct_branch" + ("" if fwd else "(adj)"), lib.ffno_dct_branch, _p(src), _p(dst), resid, _p(spec), _p(ws.SY),
                    _p(planes), _p(self._twiddle(2 * v.L)), v.Bv, v.Mv, v.Nv, C, v.K, v.a01, conj, accumulate, st)
        elif fused:      # (records its output maximum itself)
            self._k(name, lib.ffno_spectral_fused, _p(src), _p(dst), resid, _p(save), _p(planes), _p(self._twiddle(v.L)),
                    v.Bv, v.Mv, v.Nv, C, v.K, v.a01, ck_f, ck_i, conj, accumulate, rout, st)
            return
        else:
            spec, tw = save if save is not None else ws.SD, self._twiddle(v.L)
            self._k("dft_fwd", lib.ffno_dft_fwd, _p(src), _p(spec), _p(tw), v.Bv, v.Mv, v.Nv, C, v.K, v.a01, ck_f, st)
            y = spec
            if planes is not None:
                self._k("mode_mix", lib.ffno_mode_mix, _p(spec), _p(planes), _p(ws.SY), v.R, C, v.K, conj, st)
                y = ws.SY
            self._k("dft_inv", lib.ffno_dft_inv, _p(y), _p(dst), resid, _p(tw), v.Bv, v.Mv, v.Nv, C, v.K, v.a01, ck_i,
                    accumulate, st)
        self._fold(dst, rout, st)       # the stage / DCT / 2-D kernels do not record their output maximum themselves

    # ------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, save_for_backward: bool, training: Optional[bool] = None, own_output: bool = True) -> torch.Tensor:
        try:
            return self._forward(x, save_for_backward, training, own_output)
        except _StackRetry:      # (the persistent inference launch is off now: the same pass on the per-layer launches)
            return self._forward(x, save_for_backward, training, own_output)

    # ---- what the last forward pass ran (tests / bench.py); absent before the first one -------------------------------------
    def _last(self, field: str):
        if self._last_plan is None:
            raise AttributeError(field)
        return getattr(self._last_plan, field)

    paired_last = property(lambda self: self._last("conc"))      # (bench.py: which algorithmic-work table applies)
    infer_last = property(lambda self: self._last("infer"))
    infer_self_ranged_last = property(lambda self: self._last("infer_sr"))
    _saved_x3 = property(lambda self: (self._last("x3"), self._last("x3pair")))
    _x3_fmt = property(lambda self: None if self._last_plan is None else self._last_plan.x3fmt)
    _saved_lazy = property(lambda self: self._last("lazy"))
    _saved_ws = property(lambda self: None if self._saved is None else self._saved.ws)      # (the workspace backward() will use)

    def _forward(self, x: torch.Tensor, save_for_backward: bool, training: Optional[bool] = None, own_output: bool = True) -> torch.Tensor:
        """x [B, *spatial, input_dim] fp32 on the device -> [B, *spatial, output_dim] (a fresh tensor).
        ``training`` (default: save_for_backward) switches the dropout masks on (nn.Module.training of the reference).
        ``own_output=False`` returns a view of the workspace's output buffer instead of a copy -- valid until the next forward of
        this shape (FFNOTrainer.train_step consumes it at once: one copy launch less per step)."""
        if not self.params:
            raise RuntimeError("bind() parameters first")
        _lib.require_device_tensor(x, "x")
        if x.dim() != self.nd + 2 or x.shape[-1] != self.Cin:
            raise ValueError(f"x must be [B, {'M, N' if self.nd == 2 else 'X, Y, Z'}, {self.Cin}], got {tuple(x.shape)}")
        x = x.contiguous()
        B, S = x.shape[0], tuple(x.shape[1:-1])
        lib = _lib.get_lib()
        ws = self._workspace(B, S, save_for_backward)
        if self.mode != "no-fourier":
            for v in ws.views:
                if v.K > v.L // 2 + 1:
                    raise ValueError(f"modes={v.K} exceeds size//2+1 for an axis of length {v.L} "
                                     f"(the reference raises an einsum size error)")
        st = _lib.current_stream(self.device)
        self._training = bool(save_for_backward if training is None else training)
        if self._training and (self.dropout > 0.0 or self.in_dropout > 0.0):
            self._drop_calls += 1
        plan = self._last_plan = self._plan(ws, save_for_backward, st)
        self._lift_fwd(x, ws, plan, st)
        # the whole stack of self-ranged inference layers as ONE persistent launch (ffno_infer_stack: 64 x 64 images, batch x 8 = the CU
        # count; the 8 workgroups of an image run both kernels of every layer as phases): no launch boundary, no chip-wide lock step
        self.infer_stack_last = False
        if (plan.infer_sr and self.use_infer_stack and (self.timer is None or getattr(self.timer, "allow_stack", False))
                and self._run_infer_stack(ws, plan.pair, st)):
            self.infer_stack_last = True
        else:
            layer = (self._fwd_layer_infer if plan.infer else self._fwd_layer_call if plan.layer_calls else self._fwd_layer_launches)
            for l in range(self.L):
                layer(ws, plan, l, st)
        if self.use_fork:
            torch.sum(ws.YL, dim=0, out=ws.Y)     # forecast = sum of the per-layer head outputs
            self.forecast_list = [ws.YL[l].view(B, *S, self.O).clone() for l in range(self.L)]
        else:
            self._k("head_fwd", lib.ffno_head_fwd_bf16 if plan.bf16 else lib.ffno_head_fwd, _p(ws.Blast), _p(self.fold), _p(ws.Y),
                    ws.P_in, self.C, self.O, 0, ws.pm, st)
        # the workspace this pass filled (saved tensors, sign bits, range words): the backward pass and the diagnostic readers use
        # THIS object -- an attribute switched between forward() and backward() changes the workspace key, and a freshly
        # allocated workspace would hand them uninitialised memory
        self._saved = _Saved(x, B, S, ws, self._ws_key, plan) if save_for_backward else None
        y = ws.Y.view(B, *S, self.O)
        return y.clone() if own_output else y

    def _plan(self, ws, save: bool, st) -> _Plan:
        """Which kernels this pass and the backward pass over it run; prepares the weight packs in the formats chosen here."""
        lib = _lib.get_lib()
        C, H = self.C, self.H
        full = self.mode == "full"
        fused = self._can_fuse(ws.views)
        x3 = [bool(fused[w] and self._x3_ok(w, v, ws.views)) for w, v in enumerate(ws.views)]      # ... on the split kernels
        # format of the packed x3 weight sets per axis: fp16x2 where the FUSED x3 kernel mixes with them (the stage kernels of
        # the 17..32-mode axes read bf16x3 packs)
        # ... and FFNO_PLANES_FP16X2_M16 (the 16-row mix) for the many-mode axes (width 64, 17..64 modes: 4-line tiles with 8 live mix
        # rows) when their DFT-fragment tables are in use and ALL axes are such and share a tile height (a paired launch carries one
        # format and one tile height)
        many = [v.K > 16 for v in ws.views]
        m16 = bool(C == 64 and all(many) and len({v.K <= 32 for v in ws.views}) == 1)
        x3fmt = [(2 if (m16 and many[w]) else 1) if (self._x3_h2() and fused[w] and x3[w]) else 0 for w in range(len(ws.views))]
        for w, v in enumerate(ws.views):
            v.x3fmt = x3fmt[w]
        self._prepare_weights(st, x3fmt)
        singles, pair = self._schedule(fused, ws.views) if self._conc() else (list(range(len(ws.views))), None)
        if pair is not None and fused[pair[0]] and not (x3[pair[0]] and x3[pair[1]]):
            # one fused launch for two axes needs ONE kernel family to take both shapes: either both on the split (x3) kernels
            # or both on the fp32-MFMA fused kernel; an axis that is "fused" through the x3 kernels only next to one that the
            # x3 kernels refuse (x3_min_lines, a missing pack) would be handed to a kernel that does not support it
            if not all(lib.ffno_spectral_fused_supported(C, ws.views[w].K, ws.views[w].L) for w in pair):
                singles, pair = list(range(len(ws.views))), None
        conc = pair is not None
        x3pair = bool(conc and x3[pair[0]] and x3[pair[1]])
        if conc and not fused[pair[0]]:      # both axes staged: the split-bf16 stage kernels when the library takes the shape
            x3pair = bool(self.use_x3 and self.spectral == "factorized" and all(
                lib.ffno_spectral_x3_staged_supported(C, ws.views[w].K, ws.views[w].L)
                and (not full or self.xplanes[0][w] is not None) for w in pair)
                and 4 * C * max(v.Bv * v.Mv * v.Nv for v in ws.views) < 2 ** 32)
        layer_calls = bool(self.use_layer_calls and self.timer is None and conc and fused[pair[0]] and self._plain_layer)
        bwd_layer_calls = bool(self.use_layer_calls and conc and fused[pair[0]] and not singles and self._plain_layer
                               and ws.defer_reduce and self.mode != "no-fourier")
        infer = bool(not save and self._infer_ok(ws, conc, pair, singles, x3pair, fused))
        if infer and ws.MIX is None:
            ws.MIX = [torch.empty(int(lib.ffno_infer_mix_bytes(C, ws.views[w].K, ws.views[w].R)) // 4, dtype=torch.int32,
                                  device=self.device) for w in pair]
        # self-ranged inference layers (axis lengths <= 64: ffno.h FFNO_BRANCH_SELF_RANGE): the first kernel scales every line from its
        # own maximum, so no launch of this forward has to fold a range word for it (lift, second kernel: no atomics, no fold barrier)
        infer_sr = bool(infer and self.infer_self_range and all(ws.views[w].L <= 64 for w in pair))
        # both branch outputs of every layer are kept and the feed-forward does not write their sum (the deferred weight-gradient
        # launch forms it)
        lazy = bool(save and conc and ws.lazy_sums)
        bf16 = self._bf16()
        if bf16 and not (all(fused) and all(x3) and self._h2() and self._x3_h2() and self._plain_layer and self.spectral == "factorized"
                         and (C, H) in ((64, 256), (32, 128)) and full and self.dropout == 0.0 and self.in_dropout == 0.0):
            raise NotImplementedError(
                "storage='bf16' covers the fused split-kernel path of the factorized operators (2-D grids / meshes and the 3-D mesh: "
                "width 64 with up to 64 modes or width 32 with up to 16, factor 4, mode='full', fp16x2 splits, 2-layer feed-forward "
                "without fork heads / LayerNorm / dropout); this configuration runs with storage='fp32'")
        return _Plan(fused, x3, x3fmt, singles, pair, conc, x3pair, layer_calls, bwd_layer_calls, infer, infer_sr, lazy, bf16, save)

    def _lift_fwd(self, x, ws, plan: _Plan, st):
        lib = _lib.get_lib()
        lin_in = self.linears["in_proj."]
        if ws.pm is not None:
            ws.X.zero_()     # F.pad(..., 0) of the lifted features (mesh_3d.py:165)
        if self._ranged() and not plan.infer_sr:
            # the forward's words: layer inputs (x) and branch outputs (s) -- and, in the same launch, the words of the backward
            # pass that will follow this forward
            ws.RW.zero_()
            ws.rw_bwd_clean = True
        in_drop = self._training and self.in_dropout > 0.0
        self._k("lift_fwd", lib.ffno_lift_fwd_bf16 if plan.bf16 else lib.ffno_lift_fwd, _p(x), _p(lin_in.weff),
                _p(self.params["in_proj.bias"]), _p(ws.X), ws.P_in,
                self.Cin, self.C, ws.pm, None if (in_drop or plan.infer_sr) else self._rw(ws, "x", 0), st)
        if in_drop:      # x = self.drop(x) after in_proj (grid_2d.py:158): a regenerated mask over the lifted features
            self._in_drop_seed = _site_seed(self.drop_seed, self._drop_calls, 0xFFFF, 0, 2)
            self._k("in_dropout", lib.ffno_dropout, _p(ws.X), ws.X.numel(), self.in_dropout, self._in_drop_seed, st)
            self._fold(ws.X, self._rw(ws, "x", 0), st)

    def _fwd_singles(self, ws, plan: _Plan, l: int, s_l, rx, rs_, st) -> int:
        """s_l (+)= branch(x) of the axes that run on their own launches (stage-A spectra kept when training) -> how many."""
        sv, full = (l if plan.save else 0), self.mode == "full"
        for n, w in enumerate(plan.singles):
            keep = ws.SXall[w][sv] if (full and (plan.save or not plan.fused[w])) else None
            self._spectral("spectral_fused", ws, ws.views[w], ws.X, s_l, None, keep,
                           self._planes_for(self._fw_set_of[l], w, 0, plan.x3[w]), True, int(n > 0), plan.fused[w], st,
                           x3=plan.x3[w], rin=rx, rout=rs_)
        return len(plan.singles)

    def _fwd_layer_infer(self, ws, plan: _Plan, l: int, st):
        """Layer l through the two-launch inference layer (ffno_layer_infer, or its two launches as two timed calls)."""
        lib, C, H, last, si, (a, b) = _lib.get_lib(), self.C, self.H, l == self.L - 1, self._fw_set_of[l], plan.pair
        rx, _, rxn = self._rw(ws, "x", l), self._rw(ws, "s", l), self._rw(ws, "x", l + 1)
        l0, l1, b0, b1 = self._ff_weights(l)
        ba = self._branch(ws.views[a], ws.X, ws.MIX[0], None, None, self._planes_for(si, a, 0, True), 0, True, True, rx, None)
        bb = self._branch(ws.views[b], ws.X, ws.MIX[1], None, None, self._planes_for(si, b, 0, True), 0, True, True, rx, None)
        if plan.infer_sr:
            ba.flags = bb.flags = _capi.BRANCH_SELF_RANGE
            ba.in_amax = bb.in_amax = None
            rxn = None
        out_l = ws.Blast if last else ws.X
        if self.timer is None:
            d = _capi.LayerInferDesc(ba, bb, X3_INTERLEAVE, 0, _p(l0.fx[0]), _p(b0), _p(l0.fx[1]), _p(b1),
                                     None if last else _p(ws.X), _p(out_l), C, H, rxn)
            self._k("layer_infer", lib.ffno_layer_infer, ctypes.byref(d), st)
        else:       # (per-kernel timing: the two launches as two calls)
            self._k("spectral_mix", lib.ffno_spectral_x3_mix_pair, ctypes.byref(ba), ctypes.byref(bb), C, X3_INTERLEAVE, st)
            self._k("infer_ff", lib.ffno_infer_ff, ctypes.byref(ba), ctypes.byref(bb), _p(l0.fx[0]), _p(b0), _p(l0.fx[1]),
                    _p(b1), None if last else _p(ws.X), _p(out_l), C, H, rxn, st)

    def _fwd_layer_call(self, ws, plan: _Plan, l: int, st):
        """Layer l as the axes that run on their own, then ONE call for the paired branches + feed-forward (ffno_layer_fwd)."""
        save, lazy, x3pair, last = plan.save, plan.lazy, plan.x3pair, l == self.L - 1
        sv = l if save else 0
        s_l, si = ws.S[sv], self._fw_set_of[l]
        a, b = plan.pair
        rx, rs_, rxn = self._rw(ws, "x", l), self._rw(ws, "s", l), self._rw(ws, "x", l + 1)      # layer input, branch out, next
        nwrit = self._fwd_singles(ws, plan, l, s_l, rx, rs_, st) if plan.singles else 0
        keep_a, keep_b = (ws.SXall[a][sv], ws.SXall[b][sv]) if (save and self.mode == "full") else (None, None)
        l0, l1, b0, b1 = self._ff_weights(l)
        d = _capi.LayerFwdDesc(
            self._branch(ws.views[a], ws.X, s_l, None, keep_a, self._planes_for(si, a, 0, x3pair), int(nwrit > 0), x3pair, True,
                         rx, rs_),
            self._branch(ws.views[b], ws.X, ws.TS[sv] if lazy else ws.T, None, keep_b, self._planes_for(si, b, 0, x3pair), 0, x3pair,
                         True, rx, rs_),
            int(x3pair), X3_INTERLEAVE, _p(l0.fx[0]), _p(b0), _p(l0.fx[1]), _p(b1),
            _p(s_l) if (save and not lazy) else None, None if last else _p(ws.X), _p(ws.Blast if last else ws.X),
            _p(ws.MASK[sv]) if save else None, ws.P, self.C, self.H, int(self._h2()),
            int(self.ff_schedule), int(self.ff_max_workgroups), 0, 0, rxn)
        self._k("layer_fwd", _lib.get_lib().ffno_layer_fwd, ctypes.byref(d), st)

    def _fwd_layer_launches(self, ws, plan: _Plan, l: int, st):
        """Layer l as individual launches: spectral branches (single, then paired), feed-forward, LayerNorm, fork head."""
        lib, C, P, save, last = _lib.get_lib(), self.C, ws.P, plan.save, l == self.L - 1
        sv = l if save else 0
        s_l = ws.S[sv]
        rx, rs_, rxn = self._rw(ws, "x", l), self._rw(ws, "s", l), self._rw(ws, "x", l + 1)      # layer input, branch out, next
        t_l = (ws.TS[sv] if plan.lazy else ws.T) if plan.conc else None      # second branch output of a paired launch
        if self.mode == "no-fourier":
            s_l.copy_(ws.X)
            self._fold(s_l, rs_, st)
        else:
            nwrit = self._fwd_singles(ws, plan, l, s_l, rx, rs_, st)
            if plan.conc:
                si, (a, b), x3pair = self._fw_set_of[l], plan.pair, plan.x3pair
                keep = [ws.SXall[w][sv] if (self.mode == "full" and save) else None for w in plan.pair]
                self._pair("spectral_fused", ws, ws.views[a], ws.views[b], ws.X, s_l, t_l, None, keep[0], keep[1],
                           self._planes_for(si, a, 0, x3pair), self._planes_for(si, b, 0, x3pair), True, st,
                           acc0=int(nwrit > 0), fused=plan.fused[a], x3=x3pair, rin=rx, rout=rs_)
        l0, l1, b0, b1 = self._ff_weights(l)
        # FeedForward(layer_norm=True): the feed-forward writes its raw output, the LayerNorm kernel adds the residual
        ff_out = ws.TL[sv] if self.layer_norm else (ws.Blast if last else ws.X)
        ff_res = None if (self.layer_norm or last) else ws.X
        ff_rout = None if self.layer_norm else rxn     # (LayerNorm: the next layer's input is the normalised tensor)
        if self.use_fork and last:            # with fork heads the last layer's backcast only feeds the dead x_L
            pass
        elif self.general_ff:
            self._ffg_fwd(ws, self.ff_prefix[l], "backcast", l, sv, s_l, ff_res, ff_out, P, st, ff_rout)
        else:      # (a paired launch left the second branch in t_l: the chain kernel adds it, and stores the sum unless it is lazy)
            self._ffs_fwd2(s_l, t_l, s_l if (plan.conc and save and not plan.lazy) else None, ff_res, l0, b0, b1, ff_out,
                           ws.MASK[sv] if save else None, P, st, rs_, ff_rout)
        if self.layer_norm and not (self.use_fork and last):
            ln = self.ff_prefix[l] + f"layers.{self.n_ff - 1}.3."
            self._k("layernorm_fwd", lib.ffno_layernorm_fwd, _p(ws.TL[sv]), _p(self.params[ln + "weight"]),
                    _p(self.params[ln + "bias"]), None if last else _p(ws.X), _p(ws.Blast if last else ws.X), _p(ws.LNS[sv]),
                    P, C, 1e-5, st)
            if not last:
                self._fold(ws.X, rxn, st)
        if self.use_fork:
            c0, c1, cb0, cb1 = self._ff_weights(l, self.fc_prefix)
            f_raw = ws.TLF[sv] if self.layer_norm else ws.F[sv]
            if self.general_ff:
                self._ffg_fwd(ws, self.fc_prefix[l], "forecast", l, sv, s_l, None, f_raw, P, st)
            else:
                self._ffs_fwd2(s_l, None, None, None, c0, cb0, cb1, f_raw, ws.MASKF[sv] if save else None, P, st, rs_, None)
            if self.layer_norm:
                ln = self.fc_prefix[l] + f"layers.{self.n_ff - 1}.3."
                self._k("layernorm_fwd", lib.ffno_layernorm_fwd, _p(f_raw), _p(self.params[ln + "weight"]),
                        _p(self.params[ln + "bias"]), None, _p(ws.F[sv]), _p(ws.LNSF[sv]), P, C, 1e-5, st)
            self._k("head_fwd", lib.ffno_head_fwd, _p(ws.F[sv]), _p(self.fold), _p(ws.YL[l]), ws.P_in, C, self.O, 0, ws.pm, st)

    # ------------------------------------------------------------------------------------------------
    def backward(self, gy: torch.Tensor, need_dx: bool = False) -> torch.Tensor:
        """gy = dL/dout [B, *spatial, output_dim].  Fills and returns the flat gradient buffer ``gflat``
        (layout: ``param_names`` order; use ``grad_view(name)``).  ``need_dx``: also compute the gradient with respect to
        the input tensor (``self.dx``, [B, *spatial, input_dim]) -- what autograd of the reference module would hand upstream."""
        saved = self._saved_pass()
        _lib.require_device_tensor(gy, "gy")
        gy = gy.contiguous()
        ws, plan, st, L = saved.ws, saved.plan, _lib.current_stream(self.device), self.L
        if self._ranged():
            # the backward's range words (g: running gradient, d: feed-forward data gradients, t / f: LayerNorm / fork heads):
            # every fp16x2 kernel of the pass scales its operands from the maximum its producer recorded -- per layer, on the
            # device, so no growth or decay of the gradient through the layers can leave the half format's range
            if not ws.rw_bwd_clean:      # (a second backward pass over the same forward)
                ws.RW[2 * (L + 1):].zero_()
            ws.rw_bwd_clean = False
        self._head_bwd(ws, plan, gy, st)
        ws.red_jobs = []
        # deferred weight-gradient launch: (s, summed gradient, packs, words, slices) of every layer, one launch after the loop
        # (paired launches or not: the airfoil mesh -- a 32-mode axis beside a 16-mode one, two launches per layer -- ran 24 per-layer
        #  weight-gradient launches of 56 us until round 5)
        ws.wg_jobs = [] if ws.defer_wgrad else None
        if plan.lazy and ws.wg_jobs is None:
            raise RuntimeError("the forward pass left the feed-forward input sums to a deferred weight-gradient launch that this "
                               "backward pass cannot run")
        layer = self._bwd_layer_call if (plan.bwd_layer_calls and self.timer is None) else self._bwd_layer_launches
        ff_seen, cur = set(), 0
        have_g1 = False      # G1 holds the second adjoint branch's part of the running gradient (to be added to g_in)
        for l in reversed(range(L)):
            # words: gradient entering this layer, its feed-forward input, the data gradient, the gradient it hands on
            words = (self._rw(ws, "g", l), self._rw(ws, "s", l), self._rw(ws, "d", l),
                     self._rw(ws, "g", l - 1) if l > 0 else self._rw(ws, "g", L))
            if self.use_fork:
                self._bwd_forecast(ws, l, words, ff_seen, st)
            if self.use_fork and l == L - 1:
                self._bwd_fork_last(ws, plan, l, cur, words, ff_seen, st)
            else:
                have_g1 = layer(ws, plan, l, cur, have_g1, words, ff_seen, st)
            cur = (cur + 1) % len(ws.G)
        self._bwd_weight_grads(saved, cur, have_g1, need_dx, st)
        return self.gflat

    def _head_bwd(self, ws, plan: _Plan, gy, st):
        lib, C, gv, pm, o0, o1 = _lib.get_lib(), self.C, self.grad_view, ws.pm, self.linears["out.0."], self.linears["out.1."]
        if pm is not None:
            (ws.GF if self.use_fork else ws.G[0]).zero_()    # adjoint of the crop (mesh_3d.py:173)
        if self.use_fork:
            # every layer's f_l goes through the same head: d/df_l = gy . weff for all l (computed once), and the
            # head-parameter reduction sums over layers
            for l in range(self.L):
                self._k("head_bwd", lib.ffno_head_bwd, _p(ws.F[l]), _p(gy), _p(self.fold), _p(ws.GF) if l == 0 else None,
                        _p(ws.headpart), _p(ws.red if l == 0 else ws.redl), ws.P_in, C, self.O, ws.nsplit_head, pm,
                        self._rw(ws, "f", 0) if l == 0 else None, st)
                if l > 0:
                    self._k("axpy", lib.ffno_axpy, _p(ws.red), _p(ws.redl), 1.0, self.O * (C + 1), st)
        else:
            self._k("head_bwd", lib.ffno_head_bwd_bf16 if plan.bf16 else lib.ffno_head_bwd, _p(ws.Blast), _p(gy), _p(self.fold),
                    _p(ws.G[0]), _p(ws.headpart), _p(ws.red), ws.P_in, C, self.O, ws.nsplit_head, pm, self._rw(ws, "g", self.L - 1), st)
        self._k("head_param_grads", lib.ffno_head_param_grads, _p(ws.red), _p(o0.weff), _p(self.params["out.0.bias"]),
                _p(o1.weff), _p(o0.gweff), _p(gv("out.0.bias")), _p(o1.gweff), _p(gv("out.1.bias")), C, HEAD_DIM, self.O, 0, st)

    def _bwd_forecast(self, ws, l: int, words, ff_seen, st):
        """Fork heads: the forecast feed-forward of layer l (after its LayerNorm) -> its part of dL/ds."""
        lib, C, P, gv, fc = _lib.get_lib(), self.C, ws.P, self.grad_view, self.fc_prefix[l]
        _, rs_, rd, _ = words
        c0, c1, _, _ = self._ff_weights(l, self.fc_prefix)
        ds_f = ws.DS if l == self.L - 1 else ws.DSF     # last layer: the forecast path is the only contribution to ds
        rf = self._rw(ws, "f", 0)
        g_fc = ws.GF
        if self.layer_norm:      # through the forecast block's LayerNorm first
            ln = fc + f"layers.{self.n_ff - 1}.3."
            self._k("layernorm_bwd", lib.ffno_layernorm_bwd, _p(ws.TLF[l]), _p(ws.LNSF[l]), _p(self.params[ln + "weight"]),
                    _p(ws.GF), None, None, _p(ws.DTF), _p(ws.lnpart), _p(gv(ln + "weight")), _p(gv(ln + "bias")), P, C,
                    int(fc in ff_seen), st)
            g_fc, rf = ws.DTF, self._rw(ws, "f", 1)
            self._fold(ws.DTF, rf, st)
        if self.general_ff:
            self._ffg_bwd(ws, fc, "forecast", l, ws.S[l], g_fc, ds_f, int(fc in ff_seen), P, st, rd)
        else:
            self._ffs_bwd2(g_fc, None, None, ws.MASKF[l], c0, ds_f, P, st, rf, rd)
            self._ff_bwd_weights(ws, ws.S[l], None, g_fc, c0, c1, self.params[fc + "layers.0.0.bias"],
                                 gv(fc + "layers.0.0.bias"), gv(fc + "layers.1.0.bias"), int(fc in ff_seen), P, st, rs_, rf)
        ff_seen.add(fc)

    def _bwd_fork_last(self, ws, plan: _Plan, l: int, cur: int, words, ff_seen, st):
        """Fork heads, last layer: x_L is unused (zero backcast gradients), dL/ds comes from the forecast path alone."""
        gv, fp = self.grad_view, self.ff_prefix[l]
        _, _, rd, rgo = words
        g_out = ws.G[(cur + 1) % len(ws.G)]
        if fp not in ff_seen:
            for k in range(self.n_ff):
                gv(fp + f"layers.{k}.0.bias").zero_()
                self.linears[fp + f"layers.{k}.0."].gweff.zero_()
            if self.layer_norm:
                gv(fp + f"layers.{self.n_ff - 1}.3.weight").zero_()
                gv(fp + f"layers.{self.n_ff - 1}.3.bias").zero_()
            ff_seen.add(fp)
        if self.mode == "no-fourier":
            g_out.copy_(ws.DS)
            self._fold(g_out, rgo, st)
            return
        si = self._fw_set_of[l]
        for w, v in enumerate(ws.views):
            keep = ws.SDall[w][l] if self.mode == "full" else None
            self._spectral("spectral_fused(adj)", ws, v, ws.DS, g_out, None, keep, self._planes_for(si, w, 1, plan.x3[w]), False,
                           int(w > 0), plan.fused[w], st, x3=plan.x3[w], rin=rd, rout=rgo)

    def _bwd_layer_call(self, ws, plan: _Plan, l: int, cur: int, have_g1: bool, words, ff_seen, st) -> bool:
        """Layer l backward in one call (ffno_layer_bwd): FF data gradient (g_in (+)= G1), weight-gradient slices, adjoint pair."""
        lib, gv, fp, last, full = _lib.get_lib(), self.grad_view, self.ff_prefix[l], l == self.L - 1, self.mode == "full"
        g_in, g_out, g1, si, (a, b), x3pair = ws.G[cur], ws.G[(cur + 1) % len(ws.G)], ws.G1, self._fw_set_of[l], plan.pair, plan.x3pair
        rg, rs_, rd, rgo = words
        l0, l1, _, _ = self._ff_weights(l)
        part = ws.ffparts[len(ws.red_jobs)]
        if ws.wg_jobs is not None:
            ws.wg_jobs.append((ws.S[l].data_ptr(), g_in.data_ptr(), l0.fx[0].data_ptr(),
                               self.params[fp + "layers.0.0.bias"].data_ptr(), l0.fx[2].data_ptr(), part.data_ptr(),
                               rs_.value, rg.value, ws.TS[l].data_ptr() if plan.lazy else 0, 0))
        d = _capi.LayerBwdDesc(
            self._branch(ws.views[a], ws.DS, g_out, None if last else _p(g_in), ws.SDall[a][l] if full else None,
                         self._planes_for(si, a, 1, x3pair), 0, x3pair, False, rd, rgo),
            self._branch(ws.views[b], ws.DS, g1, None, ws.SDall[b][l] if full else None,
                         self._planes_for(si, b, 1, x3pair), 0, x3pair, False, rd, rgo),
            int(x3pair), X3_INTERLEAVE, _p(g_in), _p(g1) if have_g1 else None, _p(g_in),
            _p(ws.MASK[l]),
            _p(l0.fx[2]), _p(l0.fx[3]), _p(ws.DS), _p(ws.S[l]), _p(l0.fx[0]), _p(self.params[fp + "layers.0.0.bias"]),
            None if ws.wg_jobs is not None else _p(part), ws.nsplit_ff, ws.P, self.C, self.H, int(self._h2()),
            int(self.ff_schedule), int(self.ff_max_workgroups), 0, rg, rs_, rd)
        self._k("layer_bwd", lib.ffno_layer_bwd, ctypes.byref(d), st)
        ws.red_jobs.append((part.data_ptr(), l0.gweff.data_ptr(), l1.gweff.data_ptr(), gv(fp + "layers.0.0.bias").data_ptr(),
                            gv(fp + "layers.1.0.bias").data_ptr()))
        ff_seen.add(fp)
        return True

    def _bwd_layer_launches(self, ws, plan: _Plan, l: int, cur: int, have_g1: bool, words, ff_seen, st) -> bool:
        """Layer l backward as launches: LayerNorm, feed-forward (data, weights), adjoint branches.  -> G1 holds a part of g_out."""
        lib, C, P, gv, fp, last = _lib.get_lib(), self.C, ws.P, self.grad_view, self.ff_prefix[l], l == self.L - 1
        g_in, g_out, g1 = ws.G[cur], ws.G[(cur + 1) % len(ws.G)], ws.G1
        rg, rs_, rd, rgo, full = *words, self.mode == "full"
        l0, l1, _, _ = self._ff_weights(l)
        g_ff = g_in       # gradient w.r.t. the feed-forward output
        if self.layer_norm:
            # through the LayerNorm first (it also folds in the second gradient buffer of a paired adjoint launch)
            ln = fp + f"layers.{self.n_ff - 1}.3."
            two = bool(plan.conc and have_g1)
            self._k("layernorm_bwd", lib.ffno_layernorm_bwd, _p(ws.TL[l]), _p(ws.LNS[l]), _p(self.params[ln + "weight"]),
                    _p(g_in), _p(ws.G1) if two else None, _p(g_in) if two else None, _p(ws.DT), _p(ws.lnpart),
                    _p(gv(ln + "weight")), _p(gv(ln + "bias")), P, C, int(fp in ff_seen), st)
            g_ff = ws.DT
            rg = self._rw(ws, "t", l)
            self._fold(ws.DT, rg, st)
        if self.general_ff:
            self._ffg_bwd(ws, fp, "backcast", l, ws.S[l], g_ff, ws.DS, int(fp in ff_seen), P, st, rd)
        else:
            # paired launches: g_in (+)= G1 while it is staged; the sum is stored back for the weight gradient and the residual path
            two = bool(plan.conc and have_g1 and not self.layer_norm)
            self._ffs_bwd2(g_ff, g1 if two else None, g_ff if two else None, ws.MASK[l], l0, ws.DS, P, st, rg, rd)
            self._ff_bwd_weights(ws, ws.S[l], ws.TS[l] if plan.lazy else None, g_ff, l0, l1, self.params[fp + "layers.0.0.bias"],
                                 gv(fp + "layers.0.0.bias"), gv(fp + "layers.1.0.bias"), int(fp in ff_seen), P, st, rs_, rg)
        ff_seen.add(fp)
        if self.use_fork:
            self._k("axpy", lib.ffno_axpy, _p(ws.DS), _p(ws.DSF), 1.0, P * C, st)     # ds = ds(backcast) + ds(forecast)
            self._fold(ws.DS, rd, st)     # (the word already holds both addends' maxima; the sum may exceed either)
        if self.mode == "no-fourier":
            if last:
                g_out.copy_(ws.DS)
            else:
                torch.add(g_in, ws.DS, out=g_out)
            self._fold(g_out, rgo, st)
            return have_g1
        si = self._fw_set_of[l]
        resid = None if last else _p(g_in)      # G_{l-1} = G_l (residual path) + adjoint terms; last layer: none
        for n, w in enumerate(plan.singles):
            keep = ws.SDall[w][l] if full else None   # dY of every layer is kept for the dW launch
            self._spectral("spectral_fused(adj)", ws, ws.views[w], ws.DS, g_out, resid if n == 0 else None, keep,
                           self._planes_for(si, w, 1, plan.x3[w]), False, int(n > 0), plan.fused[w], st, x3=plan.x3[w], rin=rd,
                           rout=rgo)
        if plan.conc:
            a, b = plan.pair
            self._pair("spectral_fused(adj)", ws, ws.views[a], ws.views[b], ws.DS, g_out, g1,
                       None if plan.singles else resid, ws.SDall[a][l] if full else None, ws.SDall[b][l] if full else None,
                       self._planes_for(si, a, 1, plan.x3pair), self._planes_for(si, b, 1, plan.x3pair), False, st,
                       acc0=int(bool(plan.singles)), fused=plan.fused[a], x3=plan.x3pair, rin=rd, rout=rgo)
        return plan.conc

    def _bwd_weight_grads(self, saved: _Saved, cur: int, have_g1: bool, need_dx: bool, st):
        """After the layer loop: deferred feed-forward weight gradients, lift backward (dL/dx), Fourier weights, weight norm."""
        lib, ws, plan, x = _lib.get_lib(), saved.ws, saved.plan, saved.x
        C, H, L, P, gv, pm = self.C, self.H, self.L, ws.P, self.grad_view, ws.pm
        g_second = None                # second addend of the gradient that enters the lift (fp32 storage, no input gradient wanted:
        if plan.conc and have_g1:      # ffno_lift_bwd2 adds it while it stages its rows; else the sum is formed first)
            if plan.bf16:
                ws.G[cur].add_(ws.G1)      # (a torch kernel on the same stream; rounds the sum to bf16 like every stored tensor)
            elif need_dx or (self._training and self.in_dropout > 0.0):
                self._k("axpy", lib.ffno_axpy, _p(ws.G[cur]), _p(ws.G1), 1.0, P * C, st)
            else:
                g_second = ws.G1
        nsl = ws.nsplit_ff
        if ws.wg_jobs:
            nsl = ws.nsplit_ffm
            table = ws.wg_table.get(_capi.FfWgDesc, tuple(ws.wg_jobs))      # (a HOST table)
            self._k("ff_bwd_weights_partial", lib.ffno_ffh_bwd_weights_partial_multi, table, len(table), P, C, H, nsl,
                    self._st(), int(plan.lazy), st)
        if ws.defer_reduce and ws.red_jobs:
            table = ws.red_table.get(_capi.FxRedDesc, tuple(ws.red_jobs), self.device)
            self._k("ff_bwd_weights_reduce", lib.ffno_ffx_bwd_weights_reduce_batched, _p(table), len(ws.red_jobs), C, H,
                    nsl, st)
        g_fin = ws.G[cur]
        lin_in = self.linears["in_proj."]
        if self._training and self.in_dropout > 0.0:      # backward of x = self.drop(in_proj(x)): the same mask, regenerated
            self._k("in_dropout", lib.ffno_dropout, _p(g_fin), g_fin.numel(), self.in_dropout, self._in_drop_seed, st)
        if g_second is not None:
            self._k("lift_bwd", lib.ffno_lift_bwd2, _p(x), _p(g_fin), _p(g_second), _p(ws.liftpart), _p(lin_in.gweff),
                    _p(gv("in_proj.bias")), ws.P_in, self.Cin, C, ws.nsplit_lift, 0, pm, st)
        else:
            self._k("lift_bwd", lib.ffno_lift_bwd_bf16 if plan.bf16 else lib.ffno_lift_bwd, _p(x), _p(g_fin), _p(ws.liftpart),
                    _p(lin_in.gweff), _p(gv("in_proj.bias")), ws.P_in, self.Cin, C, ws.nsplit_lift, 0, pm, st)
        self.dx = None
        if need_dx:
            self.dx = torch.empty(saved.B, *saved.S, self.Cin, dtype=torch.float32, device=self.device)
            g_dx = g_fin.float() if plan.bf16 else g_fin      # (the input gradient is an fp32 tensor of the caller)
            self._k("lift_bwd_data", lib.ffno_lift_bwd_data, _p(g_dx), _p(lin_in.weff), _p(self.dx), ws.P_in, self.Cin, C, pm, st)
        multi = self.spectral != "plus" and len(self._fw_sets) == L and L > 1      # per-layer weights: one launch per axis
        if multi:
            real = int(self.spectral == "dct")
            for w, v in enumerate(ws.views):
                # slices per (layer, mode): the grid is slices x modes x LAYERS here, so the per-axis count of the shared-weight
                # launch (512 / K) would make 12 288 workgroups of 37 lines each at the airfoil shape and 384 MB of partial
                # slices for the reduce launch to read back; ~512 workgroups in all are enough
                nsf = max(1, min(-(-FW_GRAD_WGS // (v.K * L)), (v.R + 63) // 64))
                pstride = nsf * 2 * v.K * C * C
                if ws.fwpart_multi[w] is None or ws.fwpart_multi[w].numel() != L * pstride:
                    ws.fwpart_multi[w] = torch.empty(L * pstride, dtype=torch.float32, device=self.device)
                ptrs = tuple(gv(self._fw_sets[l][w]).data_ptr() for l in range(L))
                if ws.fwgrad_sig[w] != ptrs:      # (a plain int64 tensor, not a descriptor table: as it was)
                    ws.fwgrad_tab[w] = torch.tensor(ptrs, dtype=torch.int64).to(self.device)
                    ws.fwgrad_sig[w] = ptrs
                xw, dw = self._fw_words(ws, 0)
                self._k("fw_grad_partial", lib.ffno_fw_grad_partial_multi_h2, _p(ws.SXall[w]), _p(ws.SDall[w]),
                        _p(ws.fwpart_multi[w]), v.R, C, v.K, nsf, L, v.spec, v.spec, pstride, xw, dw, v.L, st)
                self._k("fw_grad_reduce", lib.ffno_fw_grad_reduce_multi, _p(ws.fwpart_multi[w]), _p(ws.fwgrad_tab[w]), L, C, v.K,
                        nsf, pstride, 0, real, st)
        for si, names in enumerate(self._fw_sets if not multi else []):
            layers = [l for l in range(L) if self._fw_set_of[l] == si]
            l0_, nl = layers[0], len(layers)
            assert layers == list(range(l0_, l0_ + nl))
            if self.spectral == "plus":
                ws.chain.fw_grad_partial(ws.SXall[0][l0_], ws.SDall[0][l0_], ws.fwpart[si][0], st, ws.nsplit_fw[0], nl)
                self._k("fw2d_grad_reduce", lib.ffno_fw2d_grad_reduce, _p(ws.fwpart[si][0]), _p(gv(names[0])),
                        _p(gv(names[1])), C, self.K, ws.nsplit_fw[0], 0, st)
                continue
            for w, n in enumerate(names):
                v = ws.views[w]
                # dW = sum over the lines of every layer that uses this weight: ONE launch per axis
                xw, dw = self._fw_words(ws, l0_) if self.spectral == "factorized" else (None, None)
                self._k("fw_grad_partial", lib.ffno_fw_grad_partial_h2, _p(ws.SXall[w][l0_]), _p(ws.SDall[w][l0_]),
                        _p(ws.fwpart[si][w]), v.R, C, v.K, ws.nsplit_fw[w], 0, nl, v.spec, v.spec, xw, dw, v.L, st)
                reduce = lib.ffno_fw_grad_reduce_real if self.spectral == "dct" else lib.ffno_fw_grad_reduce
                self._k("fw_grad_reduce", reduce, _p(ws.fwpart[si][w]), _p(gv(n)), C, v.K, ws.nsplit_fw[w], 0, st)
        if self._desc_dev is not None:
            self._k("weightnorm_bwd", lib.ffno_weightnorm_bwd, _p(self._desc_dev), self._n_desc, self._max_rows, st)


    def relu_active_sets(self) -> Dict[Tuple[str, int], torch.Tensor]:
        """Diagnostics / parity tests: the ReLU active sets of the last ``forward(save_for_backward=True)``,
        {("backcast" | "forecast", layer): uint8 [pixels of the (padded) activation buffer, hidden]} -- what
        ``threshold_backward`` of feedforward.py:17 would see.  Split-bf16 feed-forward only."""
        ws = self._saved_pass("relu_active_sets()").ws
        if self.general_ff:
            # a LIST per block: one active set per hidden activation; with dropout a dropped unit counts as inactive
            return {(kind, l): [(h > 0).to(torch.uint8) for h in ws.HG[kind][l]] for kind in ws.HG for l in range(self.L)
                    if not (kind == "backcast" and self.use_fork and l == self.L - 1)}
        lib = _lib.get_lib()
        st = _lib.current_stream(self.device)
        out = {}
        for kind, masks in (("backcast", ws.MASK), ("forecast", ws.MASKF)):
            if masks is None:
                continue
            for l in range(self.L):
                a = torch.zeros(ws.P, self.H, dtype=torch.uint8, device=self.device)
                self._k("mask_unpack", lib.ffno_ffx_mask_unpack, _p(masks[l]), _p(a), ws.P, self.C, self.H, st)
                out[(kind, l)] = a
        return out


    def dropout_keep_sets(self):
        """Diagnostics / parity tests: the dropout masks of the last training forward, regenerated from their seeds:
        {("backcast" | "forecast", layer): [keep mask (uint8 [pixels, features]) behind every linear of the block]} and
        {"in": keep mask of the lifted features} -- what nn.Dropout drew in the reference (feedforward.py:16, grid_2d.py:158)."""
        ws = self._saved_pass("dropout_keep_sets()").ws
        lib = _lib.get_lib()
        st = _lib.current_stream(self.device)
        out = {}

        def mask(n_rows, n_cols, p, seed):
            m = torch.zeros(n_rows, n_cols, dtype=torch.uint8, device=self.device)
            self._k("dropout_mask", lib.ffno_dropout_mask, _p(m), m.numel(), p, seed, st)
            return m

        if self._training and self.in_dropout > 0.0:
            out["in"] = mask(ws.P, self.C, self.in_dropout, self._in_drop_seed)
        if self._training and self.dropout > 0.0:
            for kind in (["backcast"] + (["forecast"] if self.use_fork else [])):
                for l in range(self.L):
                    out[(kind, l)] = [mask(ws.P, self.C if k == self.n_ff - 1 else self.H, *self._drop_args(l, kind, k))
                                      for k in range(self.n_ff)]
        return out


class FFNO2DEngine(FFNOEngine):
    """FNOFactorized2DBlock geometry (the 2-D entry point used by the module mirror and the tests)."""

    def __init__(self, *, modes: int, width: int, input_dim: int, n_layers: int, factor: int, share_weight: bool,
                 share_fork: bool, ff_weight_norm: bool, mode: str = "full", use_fork: bool = False, layer_norm: bool = False,
                 n_ff_layers: int = 2, dropout: float = 0.0, in_dropout: float = 0.0):
        super().__init__(modes=modes, width=width, input_dim=input_dim, n_layers=n_layers, factor=factor,
                         share_weight=share_weight, share_fork=share_fork, ff_weight_norm=ff_weight_norm, mode=mode,
                         spatial_dims=2, padding=0, output_dim=1, use_fork=use_fork, layer_norm=layer_norm,
                         n_ff_layers=n_ff_layers, dropout=dropout, in_dropout=in_dropout)
