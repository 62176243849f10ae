"""Base of the two-view pretraining criteria (losses/barlow.py, losses/vicreg.py): a loss of the
projections z1, z2 ``[N][D]`` of the two views over the GLOBAL batch, as native kernels or as a
plain-torch twin.

Called as ``criterion(feats, labels=None)`` with ``feats`` ``[2·B_l][D]`` view-major, as
``DistributedContrastiveLoss`` is. With W ranks every rank holds the same loss L and returns L / W,
so the sum over ranks is the global loss and each rank's gradient is the exact gradient of that loss
w.r.t. its own rows. ``backend="native"`` raises when the kernels cannot take the call; ``"auto"``
uses the twin then, and warns once.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
import torch.nn as nn

from ..parallel import comm


class TwoViewLoss(nn.Module):
    """A subclass sets ``name`` (for messages) and ``ops`` (the module of its native kernels:
    ``supported``, ``MIN_D``, ``MAX_D``) and defines ``native(z1, z2)`` and ``twin(z1, z2)``."""

    def __init__(self, backend: str = "auto"):
        super().__init__()
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"backend {backend!r}")
        self.backend = backend
        self._warned = False

    def _use_native(self, z1: torch.Tensor, n_total: int) -> bool:
        if self.backend == "torch":
            return False
        if self.backend == "native":
            return True     # the ops module raises on what it cannot take: never a silent fall-back
        from ..ops import _ext
        if not (z1.is_cuda and z1.dtype == torch.float32 and _ext.available()):
            return False
        if not self.ops.supported(n_total, z1.shape[1]):
            if not self._warned:
                self._warned = True
                logging.warning(f"{self.name}: N={n_total}, D={z1.shape[1]} is outside the native kernels' range "
                                f"(D = 64·j in [{self.ops.MIN_D}, {self.ops.MAX_D}]); using the torch loss")
            return False
        return True

    def forward(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        if feats.dim() != 2 or feats.shape[0] % 2:
            raise ValueError("`feats` must be [2·B][D]: view 1 of every sample, then view 2")
        b = feats.shape[0] // 2
        z1, z2 = feats[:b], feats[b:]
        w = comm.world_size()
        loss = self.native(z1, z2) if self._use_native(z1, b * w) else self.twin(z1, z2)
        return loss / w if w > 1 else loss
