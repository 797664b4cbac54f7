"""A streamed ``.npz`` writer: what the data generators (builders/synthetic.py, builders/kolmogorov_flow.py) write their files
through, some rows at a time."""
from __future__ import annotations

import os
import shutil
import tempfile
import zipfile
from typing import Dict, List

import numpy as np


class NpzStream:
    """An .npz file whose arrays are filled some rows at a time, so that host memory holds one batch and not the split: every
    array is a memory-mapped .npy file in a scratch directory beside the output, and ``close()`` packs them, stored and not
    compressed like ``np.savez``, into the .npz and returns their shapes."""

    def __init__(self, out: str, rows: int):
        self.out, self.rows, self.arrays = out, rows, {}
        self.scratch = tempfile.mkdtemp(prefix=os.path.basename(out) + ".", dir=os.path.dirname(out) or ".")

    def array(self, name: str, tail) -> np.ndarray:
        """The memory-mapped array ``name`` [rows, *tail], created on first use."""
        if name not in self.arrays:
            self.arrays[name] = np.lib.format.open_memmap(os.path.join(self.scratch, name + ".npy"), mode="w+", dtype=np.float32,
                                                          shape=(self.rows, *tail))
        return self.arrays[name]

    def put(self, name: str, row: int, block: np.ndarray):
        self.array(name, block.shape[1:])[row:row + len(block)] = block

    def abort(self):
        """Drop what was written so far; no .npz is made."""
        self.arrays.clear()
        shutil.rmtree(self.scratch, ignore_errors=True)

    def close(self) -> Dict[str, List[int]]:
        shapes = {name: list(a.shape) for name, a in self.arrays.items()}
        for a in self.arrays.values():
            a.flush()
        self.arrays.clear()
        with zipfile.ZipFile(self.out, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
            for name in shapes:
                z.write(os.path.join(self.scratch, name + ".npy"), name + ".npy")
        shutil.rmtree(self.scratch)
        return shapes
