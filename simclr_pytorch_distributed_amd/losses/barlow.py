"""Barlow Twins loss (Zbontar et al., 2021): a negative-free pretraining objective.

For the projections z1, z2 ``[N][D]`` of the two views, each column is standardised over the
batch (``BatchNorm1d(affine=False)`` in training mode: biased variance, ε = 1e-5), then

    C = ẑ1ᵀ·ẑ2 / N          L = Σ_i (C_ii − 1)² + λ·Σ_{i≠j} C_ij²

* :func:`barlow_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch``
  and the oracle's twin.
* :class:`BarlowTwinsLoss` — called as ``criterion(feats, labels=None)`` with ``feats``
  ``[2·B_l][D]`` view-major, as ``DistributedContrastiveLoss`` is. On the GPU it runs the native
  kernels (ops/barlow.py); ``backend="native"`` raises when they cannot take the call.

With W ranks N is the global batch: the column sums and C are summed over the process group
(differentiably in the twin). Every rank then holds the same L and returns L / W, so the sum over
ranks is the global loss and each rank's gradient is the exact gradient of that loss w.r.t. its
own rows, as the contrastive criterion's.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
import torch.nn as nn

from ..parallel import comm


def barlow_reference(z1: torch.Tensor, z2: torch.Tensor, lambd: float = 0.0051, eps: float = 1e-5) -> torch.Tensor:
    """The loss of the global batch from this rank's rows (differentiable; the same value on every rank)."""
    dt = torch.promote_types(torch.promote_types(z1.dtype, z2.dtype), torch.float32)
    z1, z2 = z1.to(dt), z2.to(dt)
    n = z1.shape[0] * comm.world_size()
    sums = comm.all_reduce_with_grad(torch.stack([z1.sum(0), (z1 * z1).sum(0), z2.sum(0), (z2 * z2).sum(0)]))
    mu1, mu2 = sums[0] / n, sums[2] / n
    var1 = (sums[1] / n - mu1 * mu1).clamp_min(0)
    var2 = (sums[3] / n - mu2 * mu2).clamp_min(0)
    h1 = (z1 - mu1) * torch.rsqrt(var1 + eps)
    h2 = (z2 - mu2) * torch.rsqrt(var2 + eps)
    C = comm.all_reduce_with_grad(h1.t() @ h2 / n)
    d = torch.diagonal(C)
    on = ((d - 1) ** 2).sum()
    off = (C * C).sum() - (d * d).sum()
    return on + lambd * off


class BarlowTwinsLoss(nn.Module):
    def __init__(self, lambd: float = 0.0051, eps: float = 1e-5, backend: str = "auto"):
        super().__init__()
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"backend {backend!r}")
        self.lambd = float(lambd)
        self.eps = float(eps)
        self.backend = backend
        self._warned = False

    def _use_native(self, z1: torch.Tensor, n_total: int) -> bool:
        if self.backend == "torch":
            return False
        from ..ops import _ext, barlow
        if self.backend == "native":
            return True     # ops.barlow raises on what it cannot take: never a silent fall-back
        if not (z1.is_cuda and z1.dtype == torch.float32 and _ext.available()):
            return False
        if not barlow.supported(n_total, z1.shape[1]):
            if not self._warned:
                self._warned = True
                logging.warning(f"Barlow Twins: N={n_total}, D={z1.shape[1]} is outside the native kernels' range "
                                f"(D = 64·j in [{barlow.MIN_D}, {barlow.MAX_D}]); using the torch loss")
            return False
        return True

    def forward(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        if feats.dim() != 2 or feats.shape[0] % 2:
            raise ValueError("`feats` must be [2·B][D]: view 1 of every sample, then view 2")
        b = feats.shape[0] // 2
        z1, z2 = feats[:b], feats[b:]
        w = comm.world_size()
        if self._use_native(z1, b * w):
            from ..ops import barlow
            loss = barlow.barlow_loss(z1, z2, self.lambd, self.eps)
        else:
            loss = barlow_reference(z1, z2, self.lambd, self.eps)
        return loss / w if w > 1 else loss
