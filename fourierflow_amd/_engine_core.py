"""What the host engines share: the layout of the flat parameter / gradient buffers, the validation of the tensors handed to
``bind()`` and the launch wrapper."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from . import _capi, _lib


class EngineCore:
    can_return_view = False      # forward(..., own_output=False) exists

    def _lay_out(self, param_shapes: Dict[str, Tuple[int, ...]]):
        """``param_shapes``: name -> shape in registration order, which is the order of the flat buffers."""
        self.param_shapes = {n: tuple(s) for n, s in param_shapes.items()}
        self.param_names = list(self.param_shapes)
        self._offsets, off = {}, 0
        for n in self.param_names:
            self._offsets[n] = off
            off += int(np.prod(self.param_shapes[n]))
        self.n_params = off

    def _validate(self, params: Dict[str, torch.Tensor]):
        """Every parameter present, fp32 on the device, of its shape, contiguous, all on one device -> that device."""
        missing = [n for n in self.param_names if n not in params]
        if missing:
            raise KeyError(f"missing parameters: {missing[:4]}{'...' if len(missing) > 4 else ''}")
        dev = None
        for n in self.param_names:
            t = params[n]
            _lib.require_device_tensor(t, n)
            if tuple(t.shape) != self.param_shapes[n]:
                raise ValueError(f"{n}: expected shape {self.param_shapes[n]}, got {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{n} must be contiguous")
            dev = dev or t.device
            if t.device != dev:
                raise ValueError("all parameters must live on one device")
        return dev

    def grad_view(self, name: str) -> torch.Tensor:
        o = self._offsets[name]
        return self.gflat[o:o + int(np.prod(self.param_shapes[name]))].view(self.param_shapes[name])

    def weights_changed(self):
        """Parameter memory was written behind PyTorch's back (a raw-pointer kernel): nothing derived is kept here."""

    def _k(self, name, fn, *args):
        """Enqueue one C-ABI call; with a timer attached, bracket it with HIP events on the launch stream."""
        t = self.timer
        if t is not None and hasattr(t, "seen"):      # (an optional method of the timer protocol, which is not engine state)
            t.seen(name, fn, args)          # bench.py: capture (entry point, arguments) for replay timing
        rc = fn(*args) if t is None else self._timed(name, fn, *args)
        if rc != 0:
            _capi.check(rc, name)

    def _timed(self, name, fn, *args) -> int:
        t = self.timer
        if t is None or not t.want(name):
            return fn(*args)
        t.start(name, self._issue_stream)
        rc = fn(*args)
        t.stop(name, self._issue_stream)
        return rc
