"""Zero padding / cropping of channels-last activations (fourierflow_amd/csrc/meshpad.hip: ffno_pad_embed, ffno_pad_crop,
ffno_pad_supported) through the C ABI against numpy indexing, bit for bit: what the wide mesh engine puts between its dense
lift / head and its padded layers.  CPU wave emulator (-m "not gpu") and MI355X (-m gpu)."""
import ctypes
import math

import numpy as np
import pytest

from backend_util import Backend, be  # noqa: F401

# (batch, dense sizes, per-axis pad, channels)
CASES = [
    pytest.param(2, (5, 4), (8, 8), 96, id="2d_5x4_pad8_c96"),
    pytest.param(2, (3, 4, 2), (2, 2, 2), 128, id="3d_3x4x2_pad2_c128"),
    pytest.param(2, (3, 4, 2), (1, 0, 3), 128, id="3d_unequal_pads"),
    pytest.param(3, (7,), (5,), 96, id="1d"),
    pytest.param(2, (5, 4), (3, 2), 100, id="c100_not_a_multiple_of_32"),
]


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def interior(sizes):
    return (slice(None),) + tuple(slice(0, s) for s in sizes)


def run_pair(be, B, sizes, pads, C, seed=0):
    """-> (x, y, embed(x), crop(y)) as numpy arrays; both destinations start as NaN."""
    rs = np.random.RandomState(seed)
    padded = tuple(s + p for s, p in zip(sizes, pads))
    x = rs.standard_normal((B, *sizes, C)).astype(np.float32)
    y = rs.standard_normal((B, *padded, C)).astype(np.float32)
    ex, cy = be.empty((B, *padded, C)), be.empty((B, *sizes, C))
    sz, pd = ints(sizes), ints(pads)
    assert be.lib.ffno_pad_supported(len(sizes), sz, pd, C) == 1
    assert be.lib.ffno_pad_embed(be.ptr(be.put(x)), be.ptr(ex), B, len(sizes), sz, pd, C, None) == 0
    assert be.lib.ffno_pad_crop(be.ptr(be.put(y)), be.ptr(cy), B, len(sizes), sz, pd, C, None) == 0
    return x, y, np.asarray(be.get(ex)), np.asarray(be.get(cy))


def check_pair(B, sizes, pads, C, x, y, ex, cy):
    padded = tuple(s + p for s, p in zip(sizes, pads))
    want = np.zeros((B, *padded, C), np.float32)
    want[interior(sizes)] = x
    # bit-exact, and the pad region is +0.0f in every element (the NaN the destination held is gone)
    assert np.array_equal(ex.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cy.view(np.uint32), y[interior(sizes)].view(np.uint32))
    # <embed(x), y> == <x, crop(y)> exactly: a product of two fp32 values is exact in fp64 and math.fsum rounds the exact sum once,
    # whatever the order and however many zero terms the pad region adds
    assert math.fsum((ex.astype(np.float64) * y).ravel()) == math.fsum((x.astype(np.float64) * cy).ravel())


@pytest.mark.parametrize("B,sizes,pads,C", CASES)
def test_pad_embed_and_crop_are_numpy_indexing(be, B, sizes, pads, C):
    check_pair(B, sizes, pads, C, *run_pair(be, B, sizes, pads, C, seed=len(sizes) + C))


def test_pad_supported_names_what_it_refuses(be):
    sup = be.lib.ffno_pad_supported
    assert sup(2, ints((5, 4)), ints((8, 8)), 96) == 1
    assert sup(2, ints((5, 4)), ints((0, 0)), 4) == 1
    assert sup(2, ints((5, 4)), ints((8, 8)), 98) == 0            # C % 4 != 0
    assert sup(4, ints((2, 2, 2, 2)), ints((1, 1, 1, 1)), 96) == 0      # 4 spatial dims
    assert sup(0, ints((1,)), ints((1,)), 96) == 0
    assert sup(2, ints((5, 4)), ints((8, -1)), 96) == 0            # a negative pad
    assert sup(2, ints((5, 0)), ints((8, 8)), 96) == 0
    # ... and the entry points return the codes of include/ffno.h instead of launching
    x, out = be.zeros((1, 5, 4, 96)), be.empty((1, 13, 12, 96))
    for fn, a, b in ((be.lib.ffno_pad_embed, x, out), (be.lib.ffno_pad_crop, out, x)):
        assert fn(be.ptr(a), be.ptr(b), 1, 2, ints((5, 4)), ints((8, -1)), 96, None) == -2
        assert fn(be.ptr(a), be.ptr(b), 1, 4, ints((5, 4, 1, 1)), ints((8, 8, 0, 0)), 96, None) == -2
        assert fn(be.ptr(a), be.ptr(b), 0, 2, ints((5, 4)), ints((8, 8)), 96, None) == -1
        assert fn(None, be.ptr(b), 1, 2, ints((5, 4)), ints((8, 8)), 96, None) == -1
    assert np.isnan(np.asarray(be.get(out))).all()


@pytest.mark.gpu
def test_pad_grid_stride_loop_turns_over_on_gpu():
    """The launch is min(ceil(float4 elements / 256), 2048) blocks of 256 threads (csrc/meshpad.hip: kPadBlock, kPadMaxBlocks), so
    one sweep of the grid covers 2048 * 256 = 524288 float4 elements of the destination.  Both destinations here exceed one sweep
    and neither is a multiple of it -- padded 6 x 69 x 58 x 32 = 768384, dense 6 x 61 x 50 x 32 = 585600 float4 -- so every thread
    advances its mixed-radix counter at least once, most carry between digits, and the last sweep is partial."""
    B, sizes, pads, C = 6, (61, 50), (8, 8), 128
    sweep = 2048 * 256
    n_dense, n_padded = B * 61 * 50 * C // 4, B * 69 * 58 * C // 4
    assert sweep < n_dense < 2 * sweep and sweep < n_padded < 2 * sweep and n_dense % sweep and n_padded % sweep
    check_pair(B, sizes, pads, C, *run_pair(Backend("gpu"), B, sizes, pads, C, seed=7))
