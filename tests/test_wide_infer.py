"""The forward-only pass of the wide engine (fourierflow_amd/engine_wide.py, widths 96 .. 256): with ``fuse_ff`` it records one
fused feed-forward launch per layer (csrc/bgemm_ff.hip) in place of wide_ff1 + wide_ff2, gives the bits of the training forward
and keeps no [pixels, hidden] tensor; without it, and in every pass that saves for the backward pass, the launches are the
pair's.  CPU wave emulator (-m "not gpu") and MI355X (-m gpu)."""
import pytest
import torch

import golden_util as gu
from backend_util import host_device  # noqa: F401
from test_wide_block import build_block
from test_wide_mesh import build_model, make_io

BLOCK = dict(modes=3, width=96, n_layers=2, factor=4, input_dim=3, gain=0.1)
_MESH = dict(width=96, n_layers=2, n_ff_layers=2, layer_norm=False, factor=4, share_weight=False, ff_weight_norm=True)
# name -> (kind, module keywords, seed, batch, data grid); the mesh modules pad by 8: 13 x 15 and 13 x 12 x 11
CASES = {
    "block_shared_wnorm": ("block", dict(BLOCK, share_weight=True, ff_weight_norm=True), 51, 2, (8, 12)),
    "block_unshared_plain": ("block", dict(BLOCK, share_weight=False, ff_weight_norm=False), 52, 2, (8, 12)),
    "mesh2d_5x7_pad8": ("mesh", dict(_MESH, modes_x=3, modes_y=2, input_dim=4), 53, 2, (5, 7)),
    "mesh3d_5x4x3_pad8": ("mesh", dict(_MESH, modes_x=2, modes_y=3, modes_z=2, input_dim=5, output_dim=4), 54, 1, (5, 4, 3)),
}


def build(tag, device, fuse_ff=True):
    """-> (module, bound engine with ``fuse_ff`` set before its first pass, the engine's input: the mesh modules append their
    coordinate channels)."""
    kind, kw, seed, B, S = CASES[tag]
    if kind == "block":
        blk = build_block(kw, seed, device)
        x_np = gu.make_block_io(kw, seed, B, *S)[0]
    else:
        blk = build_model(kw, seed, device, padding=8)
        x_np = make_io(kw, seed, B, S)[0]
    eng = blk._engine_for([p for _, p in blk.engine_parameters()])
    eng.fuse_ff = fuse_ff
    return blk, eng, blk.prepare_input(torch.from_numpy(x_np).to(device))


def names(ws):
    return [o[0] for o in ws.fwd]


def pair_names(eng):
    """What a pass records today: lift, per layer the three launches of every axis (the last axis first) and the feed-forward
    pair, head; the mesh operators pad after the lift and crop before the head."""
    axes = [eng.axis_of_weight.index(d) for d in reversed(range(eng.nd))]
    layer = [f"wide_{op}{w}" for w in axes for op in ("dft", "mix", "idft")] + ["wide_ff1", "wide_ff2"]
    pad = eng.pad > 0
    return (["wide_lift"] + ["wide_pad_embed"] * pad + layer * eng.L + ["wide_pad_crop"] * pad + ["wide_head0", "wide_head1"])


def ws_bytes(ws):
    """The bytes of every tensor the workspace owns (each counted once; the recorded passes only refer to them and to the
    parameters)."""
    seen = {}

    def walk(v):
        if isinstance(v, torch.Tensor):
            seen[id(v)] = v.numel() * v.element_size()
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
    for k, v in vars(ws).items():
        if k not in ("fwd", "bwd", "bwd_dx"):
            walk(v)
    return sum(seen.values())


@pytest.mark.parametrize("tag", list(CASES))
def test_fused_forward_only_pass_gives_the_training_forward_bits(host_device, tag):
    _, eng, x = build(tag, host_device)
    B, S = x.shape[0], tuple(x.shape[1:-1])
    y_infer = eng.forward(x, False)
    y_train = eng.forward(x, True)
    assert torch.equal(y_infer, y_train)
    ws, ws_save = eng._workspace(B, S, False), eng._workspace(B, S, True)
    got = names(ws)
    assert got.count("wide_ff") == eng.L and "wide_ff1" not in got and "wide_ff2" not in got
    want = pair_names(eng)
    assert names(ws_save) == want
    # the same pass but for the feed-forward launches
    assert [n for n in got if n != "wide_ff"] == [n for n in want if n not in ("wide_ff1", "wide_ff2")]
    # memory: no hidden image, and the helper states both workspaces without allocating them
    P, H = ws.P, eng.H
    assert P == B * int(torch.tensor([s + eng.pad for s in S]).prod())
    assert not any(t.numel() >= P * H for t in ws.Hh)
    assert len(ws_save.Hh) == eng.L and all(tuple(t.shape) == (P, H) for t in ws_save.Hh)
    fused_bytes, pair_bytes = eng.forward_workspace_bytes(B, *S, fused=True), eng.forward_workspace_bytes(B, *S, fused=False)
    assert fused_bytes == pair_bytes - 4 * P * H
    assert fused_bytes == ws_bytes(ws) == eng.forward_workspace_bytes(B, *S)
    eng.fuse_ff = False
    assert pair_bytes == ws_bytes(eng._workspace(B, S, False)) == eng.forward_workspace_bytes(B, *S)


@pytest.mark.parametrize("tag", ["block_shared_wnorm", "mesh2d_5x7_pad8"])
def test_fuse_ff_off_records_the_pair(host_device, tag):
    _, eng, x = build(tag, host_device, fuse_ff=False)
    B, S = x.shape[0], tuple(x.shape[1:-1])
    y_infer = eng.forward(x, False)
    ws = eng._workspace(B, S, False)
    assert names(ws) == pair_names(eng)
    assert len(ws.Hh) == 1 and tuple(ws.Hh[0].shape) == (ws.P, eng.H)
    assert torch.equal(y_infer, eng.forward(x, True))
    # read when a pass is recorded: the pair's pass stays, the fused one is recorded beside it
    eng.fuse_ff = True
    assert torch.equal(eng.forward(x, False), y_infer)
    assert "wide_ff" in names(eng._workspace(B, S, False)) and names(ws) == pair_names(eng)


def test_fused_pass_through_the_public_module(host_device):
    """FNOFactorized2DBlock in eval() under no_grad reaches the fused pass and gives the training-mode forecast bit for bit;
    a backward pass after it is refused as after any forward that saved nothing."""
    blk, eng, x = build("block_shared_wnorm", host_device)
    assert eng is blk.engine() and eng.fuse_ff is True
    blk.train()
    train = blk(x)["forecast"].detach().clone()
    assert train.requires_grad is False and eng._saved is not None
    blk.eval()
    with torch.no_grad():
        infer = blk(x)["forecast"]
    assert torch.equal(infer, train)
    assert "wide_ff" in names(eng._last) and eng._last.saves is False
    with pytest.raises(RuntimeError, match=r"needs a preceding forward\(save_for_backward=True\)"):
        eng.backward(torch.ones_like(infer))


def test_fuse_ff_default_follows_the_nearest_measured_width():
    from fourierflow_amd.engine_wide import FUSE_FF_MEASURED, WIDE_WIDTHS, WideFFNO2DEngine, fuse_ff_default
    assert set(FUSE_FF_MEASURED) == {96, 128}
    for w in WIDE_WIDTHS:
        assert fuse_ff_default(w) is FUSE_FF_MEASURED[96 if w == 96 else 128]
        eng = WideFFNO2DEngine(modes=3, width=w, input_dim=3, n_layers=1, factor=2, share_weight=True)
        assert eng.fuse_ff is fuse_ff_default(w)
