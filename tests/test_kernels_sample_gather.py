"""ffno_sample_gather (include/ffno.h) through the C ABI against numpy indexing, on the emulator and on the GPU.  The kernel only
copies, so every comparison is `assert_array_equal`, no tolerance.  Destinations are NaN-prefilled and compared WHOLE: what a
launch does not address must still be NaN.  Every layout case runs alone and with a second, unrelated field in the same launch."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from backend_util import be  # noqa: F401
from fourierflow_amd._capi import GatherField


def _rand(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


class Field:
    """One descriptor: `src` (numpy, any shape, flattened on upload), the destination's flat length per batch and a function
    giving the expected destination [B, ...] from the ids by numpy indexing.  `dst_shift` / `src_shift` move the base pointers by
    that many floats into a larger allocation (alignment cases)."""

    def __init__(self, src, dst_shape, want, Q, R, src_strides, dst_strides, src_shift=0, dst_shift=0):
        self.src, self.dst_shape, self.want, self.Q, self.R = src, dst_shape, want, Q, R
        self.src_strides, self.dst_strides, self.src_shift, self.dst_shift = src_strides, dst_strides, src_shift, dst_shift


def plain(src):
    """[n, ...] contiguous rows copied as they are."""
    L = int(np.prod(src.shape[1:]))
    return Field(src, src.shape[1:], lambda ids: src[ids], 1, L, (L, 0, 0, 1), (L, 0, 0, 1))


def run(be, fields, ids, n, B=None):
    """One launch -> (rc, [whole destination arrays, shift floats of slack in front included])."""
    lib, p = be.lib, be.ptr
    ids = np.asarray(ids, np.int32)
    B = len(ids) if B is None else B
    descs = (GatherField * len(fields))()
    srcs, dsts = [], []      # the descriptors hold raw addresses: every operand stays referenced until the results are read
    for d, f in zip(descs, fields):
        src = be.put(np.concatenate([np.full(f.src_shift, np.nan, np.float32), f.src.ravel()]))
        dst = be.empty((f.dst_shift + len(ids) * int(np.prod(f.dst_shape)),))
        srcs.append(src)
        dsts.append(dst)
        d.src = p(src).value + 4 * f.src_shift
        d.dst = p(dst).value + 4 * f.dst_shift
        d.src_sample, d.src_offset, d.src_q, d.src_r = f.src_strides
        d.dst_sample, d.dst_offset, d.dst_q, d.dst_r = f.dst_strides
        d.Q, d.R = f.Q, f.R
    dev_ids = be.put(ids)
    rc = lib.ffno_sample_gather(ctypes.cast(descs, ctypes.c_void_p), len(fields), p(dev_ids), n, B, None)
    out = [be.get(d) for d in dsts]
    del srcs, dev_ids
    return rc, out


def want_of(f, ids, keep=None):
    """The whole expected destination: the slack in front stays NaN, so do the samples of `keep`-less (bad) ids."""
    ids = np.asarray(ids)
    ok = np.ones(len(ids), bool) if keep is None else np.asarray(keep)
    w = np.full((len(ids),) + tuple(f.dst_shape), np.nan, np.float32)
    if ok.any():
        w[ok] = f.want(ids[ok])
    return np.concatenate([np.full(f.dst_shift, np.nan, np.float32), w.ravel()])


def check(be, fields, ids, n):
    rc, got = run(be, fields, ids, n)
    assert rc == 0
    for k, (f, g) in enumerate(zip(fields, got)):
        assert_array_equal(g, want_of(f, ids), err_msg=f"field {k}")


# ---- the layout cases of the three builders -------------------------------------------------------------------
def case_plain_rows():
    return [plain(_rand(1, 5, 7))], [4, 0, 4, 2], 5               # the last row, a repeated id


def case_short_rows():
    return [plain(_rand(2, 6, 1)), plain(_rand(3, 6, 42))], [5, 0, 3], 6


def case_single_sample():
    return [plain(_rand(4, 5, 7))], [3], 5


def case_interleave():
    """x1, x2 [4, 5, 3] -> [B, 5, 3, 2] (StructuredMesh2DBuilder: torch.stack([x1, x2], dim=-1))."""
    x1, x2 = _rand(5, 4, 5, 3), _rand(6, 4, 5, 3)
    want = lambda ids: np.stack([x1, x2], -1)[ids]      # noqa: E731
    # each source fills its own channel of ONE destination (test_interleave hands both the same allocation)
    f1 = Field(x1, (5, 3, 2), None, 15, 1, (15, 0, 1, 0), (30, 0, 2, 0))
    f2 = Field(x2, (5, 3, 2), None, 15, 1, (15, 0, 1, 0), (30, 1, 2, 0))
    return (f1, f2, want), [3, 1, 0, 3, 2], 4


def case_channel_pick():
    """sigma[:, 2] of [4, 3, 5, 3] (StructuredMesh2DBuilder: np.load(sigma_path)[:, output_dim])."""
    s = _rand(7, 4, 3, 5, 3)
    return [Field(s, (5, 3, 1), lambda ids: s[ids, 2][..., None], 1, 15, (45, 30, 0, 1), (15, 0, 0, 1))], [2, 3, 0], 4


def case_broadcast():
    """[n, 6] -> [B, 6, 3 * 2, 1] (PlasticityBuilder: repeat(x, 'b s1 -> b s1 s2 t 1'))."""
    x = _rand(8, 5, 6)
    want = lambda ids: np.broadcast_to(x[ids][:, :, None, None], (len(ids), 6, 6, 1))      # noqa: E731
    return [Field(x, (6, 6, 1), want, 6, 6, (6, 0, 1, 0), (36, 0, 6, 1))], [4, 1, 1, 0], 5


def case_sample_axis_last():
    """xy [9, 2, 7] -> [B, 9, 2] (ElasticityBuilder: permute(2, 0, 1)), straight from the file's layout."""
    xy = _rand(9, 9, 2, 7)
    return [Field(xy, (9, 2), lambda ids: np.transpose(xy, (2, 0, 1))[ids], 9, 2, (1, 0, 14, 7), (18, 0, 2, 1))], [6, 0, 3, 6], 7


def case_real_odd_row():
    """221 x 51 = 11271 floats at B = 3: longer than one pass of a workgroup, not a multiple of 4.  Only a sample whose id and
    whose place in the batch are both multiples of 4 starts 16-byte aligned on both sides: the first one here; the other two
    take 4-byte accesses."""
    return [plain(_rand(10, 4, 221, 51))], [0, 3, 2], 4


def case_rows_of_rows():
    """Contiguous inner runs whose rows are a multiple of 4 floats apart on both sides but not back to back: Q = 3 rows of R = 10
    out of a pitch of 12 (two 16-byte accesses and a tail of 2 per row); the last 2 floats of every destination row are not
    addressed."""
    s = _rand(11, 4, 3, 12)

    def want(ids):
        w = np.full((len(ids), 3, 12), np.nan, np.float32)
        w[:, :, :10] = s[ids][:, :, :10]
        return w

    return [Field(s, (3, 12), want, 3, 10, (36, 0, 12, 1), (36, 0, 12, 1))], [1, 3, 0], 4


SECOND = plain(_rand(99, 9, 5))      # the unrelated field (its ids are the case's own: every case has n <= 9)

CASES = [case_plain_rows, case_short_rows, case_single_sample, case_channel_pick, case_broadcast, case_sample_axis_last,
         case_real_odd_row, case_rows_of_rows]


@pytest.mark.parametrize("second", [False, True], ids=["alone", "with_second_field"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__[5:])
def test_layouts(be, case, second):
    fields, ids, n = case()
    check(be, list(fields) + ([SECOND] if second else []), ids, n)


@pytest.mark.parametrize("second", [False, True], ids=["alone", "with_second_field"])
def test_interleave(be, second):
    (f1, f2, want), ids, n = case_interleave()
    # the two fields write the two channels of ONE destination: hand both the same allocation
    lib, p = be.lib, be.ptr
    fields = [f1, f2] + ([SECOND] if second else [])
    descs = (GatherField * len(fields))()
    x1, x2, s = be.put(f1.src), be.put(f2.src), be.put(SECOND.src)
    dst, dst2 = be.empty((len(ids), 5, 3, 2)), be.empty((len(ids), 5))
    for d, f, src, out in zip(descs, fields, (x1, x2, s), (dst, dst, dst2)):
        d.src, d.dst = p(src).value, p(out).value
        d.src_sample, d.src_offset, d.src_q, d.src_r = f.src_strides
        d.dst_sample, d.dst_offset, d.dst_q, d.dst_r = f.dst_strides
        d.Q, d.R = f.Q, f.R
    assert lib.ffno_sample_gather(ctypes.cast(descs, ctypes.c_void_p), len(fields), p(be.put(np.asarray(ids, np.int32))), n,
                                  len(ids), None) == 0
    assert_array_equal(be.get(dst), want(np.asarray(ids)))
    if second:
        assert_array_equal(be.get(dst2), SECOND.src[ids])
    else:
        assert np.isnan(be.get(dst2)).all()


@pytest.mark.parametrize("second", [False, True], ids=["alone", "with_second_field"])
@pytest.mark.parametrize("src_offset,src_shift,dst_shift", [(1, 0, 0), (0, 0, 1), (0, 1, 0), (0, 0, 0)],
                         ids=["src_offset_1", "dst_base_4_bytes_off", "src_base_4_bytes_off", "aligned"])
def test_unaligned_vector_candidate(be, src_offset, src_shift, dst_shift, second):
    """A contiguous row of 16 floats is a candidate for 16-byte accesses; one float of offset on either side takes it off 16-byte
    alignment, and the wide path must step aside (a misaligned 16-byte access would fault or copy the wrong floats)."""
    s = _rand(12, 5, 20)
    f = Field(s, (16,), lambda ids: s[ids, src_offset:src_offset + 16], 1, 16, (20, src_offset, 0, 1), (16, 0, 0, 1),
              src_shift=src_shift, dst_shift=dst_shift)
    check(be, [f] + ([SECOND] if second else []), [4, 0, 2, 2], 5)


@pytest.mark.parametrize("second", [False, True], ids=["alone", "with_second_field"])
def test_out_of_range_ids_keep_their_prefill(be, second):
    n = 5
    s = _rand(13, n, 221, 3)
    fields = [plain(s)] + ([SECOND] if second else [])
    ids = [3, -1, 0, n, 4]
    rc, got = run(be, fields, ids, n)
    assert rc == 0
    keep = [True, False, True, False, True]
    for f, g in zip(fields, got):
        assert_array_equal(g, want_of(f, ids, keep))


def test_host_rejections(be):
    lib, p = be.lib, be.ptr
    a, out, ids = be.zeros((64,)), be.zeros((64,)), be.put(np.zeros(4, np.int32))

    def call(n_fields=1, ids=ids, n=4, B=4, fields="own", **kw):
        descs = (GatherField * 9)()
        for d in descs:
            d.src, d.dst = p(a).value, p(out).value
            d.src_sample = d.dst_sample = 4
            d.src_r = d.dst_r = 1
            d.Q, d.R = 1, 4
            for k, v in kw.items():
                setattr(d, k, v)
        return lib.ffno_sample_gather(ctypes.cast(descs, ctypes.c_void_p) if fields == "own" else fields, n_fields, p(ids), n, B, None)

    assert call() == 0
    assert call(n_fields=8) == 0
    assert call(ids=None) == -1 and call(fields=None) == -1
    assert call(n_fields=0) == -1 and call(n_fields=9) == -1 and call(n_fields=-1) == -1
    for name in ("B", "n"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    for name in ("Q", "R"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    assert call(src=None) == -1 and call(dst=None) == -1
    assert call(src_q=-1) == -1 and call(dst_offset=-1) == -1
    assert call(B=65536) == -2


def test_two_calls_are_bit_identical(be):
    fields, ids, n = case_real_odd_row()
    _, a = run(be, fields, ids, n)
    _, b = run(be, fields, ids, n)
    assert a[0].tobytes() == b[0].tobytes()
