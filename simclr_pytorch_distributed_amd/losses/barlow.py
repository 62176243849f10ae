"""Barlow Twins loss (Zbontar et al., 2021): a negative-free pretraining objective.

For the projections z1, z2 ``[N][D]`` of the two views, each column is standardised over the
batch (``BatchNorm1d(affine=False)`` in training mode: biased variance, ε = 1e-5), then

    C = ẑ1ᵀ·ẑ2 / N          L = Σ_i (C_ii − 1)² + λ·Σ_{i≠j} C_ij²

* :func:`barlow_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch``
  and the oracle's twin.
* :class:`BarlowTwinsLoss` — the criterion (losses/twoview.py); on the GPU it runs the native
  kernels (ops/barlow.py).

With W ranks N is the global batch: the column sums and C are summed over the process group
(differentiably in the twin).
"""
from __future__ import annotations

import torch

from ..ops import barlow
from ..parallel import comm
from .twoview import TwoViewLoss


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


class BarlowTwinsLoss(TwoViewLoss):
    name, ops = "Barlow Twins", barlow

    def __init__(self, lambd: float = 0.0051, eps: float = 1e-5, backend: str = "auto"):
        super().__init__(backend)
        self.lambd = float(lambd)
        self.eps = float(eps)

    def native(self, z1, z2):
        return barlow.barlow_loss(z1, z2, self.lambd, self.eps)

    def twin(self, z1, z2):
        return barlow_reference(z1, z2, self.lambd, self.eps)
