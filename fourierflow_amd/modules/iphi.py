"""IPhi -- MI355X-native mirror of ``fourierflow.modules.iphi.IPhi`` (reference modules/iphi.py:6-58), the coordinate
deformation network of the elasticity F-FNO.

Same constructor, parameter names / shapes and registration order (``fc_no_code`` included, for state-dict parity), same
forward contract ``forward(x [B, N, 2], code [B, 42]) -> xi [B, N, 2]``.  ``center`` and ``B`` are plain attributes like the
reference's.  Underneath: one HIP launch forward, five backward (csrc/ffno_iphi.h).  HIP only: CPU tensors raise.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _capi


class IPhi(nn.Module):
    def __init__(self, width=32):
        super().__init__()
        if width % 4:
            raise ValueError(f"IPhi: width must be a multiple of 4, got {width}")
        self.width = width
        self.fc0 = nn.Linear(4, width)
        self.fc_code = nn.Linear(42, width)
        self.fc_no_code = nn.Linear(3 * width, 4 * width)
        self.fc1 = nn.Linear(4 * width, 4 * width)
        self.fc2 = nn.Linear(4 * width, 4 * width)
        self.fc3 = nn.Linear(4 * width, 4 * width)
        self.fc4 = nn.Linear(4 * width, 2)
        self.activation = torch.tanh
        self.center = torch.tensor([0.0001, 0.0001]).reshape(1, 1, 2)
        self.B = np.pi * torch.pow(2, torch.arange(0, width // 4, dtype=torch.float)).reshape(1, 1, 1, width // 4)

    def kernel_parameters(self):
        """The twelve tensors the kernels read, in ``ffno_iphi_params`` order."""
        named = dict(self.named_parameters())
        return [named[n] for n in _capi.IPhiParams.NAMES]

    def forward(self, x, code=None):
        from ..ops import iphi_forward
        if code is None:
            raise NotImplementedError("IPhi(code=None): the fc_no_code branch (reference iphi.py:48) has no kernel; every "
                                      "shipped elasticity config passes the 42 geometry features")
        return iphi_forward(x, code, self.width, self.kernel_parameters())
