"""A set of samples held on the device as named fields, and its batches -- the counterpart of the reference's
``DataLoader(dataset, shuffle=..., drop_last=False)`` over its map-style datasets (builders/structured_mesh_2d.py:73-85,
plasticity.py:68-80, elasticity.py:76-90), without the host-side indexing, collation and upload of every batch.

Every field is uploaded once, as the set's own copy.  A field names the layout of its source and of its place in the batch
(``Field``: the strides of ``ffno_sample_gather``, include/ffno.h), so the layout change that the reference's builders make on the
host -- stack, channel pick, repeat, permute -- happens in the copy.  An epoch is a permutation of the ``n`` sample ids, uploaded
once as int32; each batch is ONE ``ffno_sample_gather`` launch for all fields, reading its ids through a pointer into that array:
a step costs no host work beyond the launch.

Order, drop-last and data parallel: the schedule of ``DeviceEpochs`` (builders/device_epochs.py) over the ``n`` sample ids;
``shuffle=False`` is file order.
"""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _capi, _lib
from .device_epochs import DeviceEpochs, tensor, upload


class Field(NamedTuple):
    """One destination of a batch: ``out`` names the batch tensor ``[B, *shape]`` it is written into (several fields may share one:
    the two channels of the airfoil ``x``), ``source`` the array it is read from.  For q < Q, r < R, in floats:
        batch[out][b].flat[dst_offset + q dst_q + r dst_r] = source.flat[id src_sample + src_offset + q src_q + r src_r]"""
    out: str
    source: object
    shape: Tuple[int, ...]
    Q: int
    R: int
    src: Tuple[int, int, int, int]      # sample, offset, q, r
    dst: Tuple[int, int, int]           # offset, q, r  (the sample stride is prod(shape))


def rows(out: str, source, shape: Optional[Sequence[int]] = None) -> Field:
    """``source [n, ...]`` copied as it is: contiguous per-sample rows; `shape` is the batch's shape of one sample."""
    L = 1
    for s in source.shape[1:]:
        L *= int(s)
    return Field(out, source, tuple(shape if shape is not None else source.shape[1:]), 1, L, (L, 0, 0, 1), (0, 0, 1))


def broadcast(out: str, source) -> Field:
    """One row that every sample of the batch receives (sample stride 0): the `times` the reference's datasets attach to each item."""
    L = int(source.size)
    return Field(out, source, (L,), 1, L, (0, 0, 0, 1), (0, 0, 1))


class DeviceSampleData(DeviceEpochs):
    def __init__(self, fields: Sequence[Field], n: int, *, device, batch_size: int, seed: int = 0, shuffle: bool = True,
                 drop_last: bool = False, rank: int = 0, world: int = 1):
        super().__init__(device=device, batch_size=batch_size, seed=seed, shuffle=shuffle, drop_last=drop_last, rank=rank,
                         world=world)
        if not 1 <= len(fields) <= _capi.GATHER_MAX_FIELDS:
            raise ValueError(f"a set has 1 to {_capi.GATHER_MAX_FIELDS} fields (one launch draws them all), got {len(fields)}")
        if not 1 <= n <= 2 ** 31 - 1:
            raise ValueError(f"a set holds 1 to 2^31 - 1 samples (int32 ids), got {n}")
        self.n = int(n)
        self.fields, self.shapes, uploaded = [], {}, {}
        for f in fields:
            key = id(f.source)
            if key not in uploaded:      # a source that several fields read is uploaded once
                uploaded[key] = upload(tensor(f.source, f.out), self.device)
            src = uploaded[key]
            size = 1
            for s in f.shape:
                size *= int(s)
            if self.shapes.setdefault(f.out, tuple(int(s) for s in f.shape)) != tuple(int(s) for s in f.shape):
                raise ValueError(f"{f.out}: fields that share a batch tensor must agree on its shape")
            if f.Q < 1 or f.R < 1 or min(f.src) < 0 or min(f.dst) < 0:
                raise ValueError(f"{f.out}: Q and R are at least 1, strides and offsets at least 0")
            # the kernel trusts its descriptors: the last float either side touches must lie inside the arrays
            last_src = (self.n - 1) * f.src[0] + f.src[1] + (f.Q - 1) * f.src[2] + (f.R - 1) * f.src[3]
            last_dst = f.dst[0] + (f.Q - 1) * f.dst[1] + (f.R - 1) * f.dst[2]
            if last_src >= src.numel() or last_dst >= size:
                raise ValueError(f"{f.out}: the field reaches float {last_src} of a source of {src.numel()} and float {last_dst} of a "
                                 f"sample of {size}")
            self.fields.append((f, src, size))
        self._schedule(self.n, "samples", self.fields[0][1])
        self._descs = (_capi.GatherField * len(self.fields))()
        for d, (f, src, size) in zip(self._descs, self.fields):
            d.src = src.data_ptr()
            d.src_sample, d.src_offset, d.src_q, d.src_r = f.src
            d.dst_sample = size
            d.dst_offset, d.dst_q, d.dst_r = f.dst
            d.Q, d.R = f.Q, f.R

    def _gather(self, ids: ctypes.c_void_p, B: int) -> Dict[str, torch.Tensor]:
        """The batch of B sample ids: one launch for all fields."""
        b = {name: torch.empty(B, *shape, dtype=torch.float32, device=self.device) for name, shape in self.shapes.items()}
        for d, (f, _, _) in zip(self._descs, self.fields):
            d.dst = b[f.out].data_ptr()
        rc = _lib.get_lib().ffno_sample_gather(ctypes.cast(self._descs, ctypes.c_void_p), len(self.fields), ids, self.n, B,
                                               _lib.current_stream(self.device))
        _capi.check(rc, "sample_gather")
        return b
