"""VICReg loss (Bardes, Ponce, LeCun, 2022): variance-invariance-covariance regularisation, a
negative-free pretraining objective that needs neither a standardised cross-correlation nor a
large batch.

For the projections z1, z2 ``[N][D]`` of the two views, with x̄_v = z_v − μ_v (column-centred):

    C_v   = x̄_vᵀ·x̄_v / (N − 1)                 S_v,j = sqrt(C_v[j][j] + ε)      (unbiased, ε = 1e-4)
    L_sim = Σ (z1 − z2)² / (N·D)
    L_std = ½·Σ_v mean_j relu(1 − S_v,j)
    L_cov = Σ_v Σ_{j≠k} C_v[j][k]² / D
    L     = λ·L_sim + μ·L_std + ν·L_cov          (λ, μ, ν) = (25, 25, 1)

* :func:`vicreg_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch``
  and the oracle's twin.
* :class:`VICRegLoss` — called as ``criterion(feats, labels=None)`` with ``feats`` ``[2·B_l][D]``
  view-major, as ``DistributedContrastiveLoss`` is. On the GPU it runs the native kernels
  (ops/vicreg.py); ``backend="native"`` raises when they cannot take the call.

With W ranks N is the global batch: the column sums, the invariance sum and C are summed over the
process group (differentiably in the twin). Every rank then holds the same L and returns L / W, so
the sum over ranks is the global loss and each rank's gradient is the exact gradient of that loss
w.r.t. its own rows, as the contrastive criterion's.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
import torch.nn as nn

from ..parallel import comm


def vicreg_reference(z1: torch.Tensor, z2: torch.Tensor, sim: float = 25.0, std: float = 25.0, cov: float = 1.0,
                     eps: float = 1e-4) -> torch.Tensor:
    """The loss of the global batch from this rank's rows (differentiable; the same value on every rank)."""
    dt = torch.promote_types(torch.promote_types(z1.dtype, z2.dtype), torch.float32)
    z1, z2 = z1.to(dt), z2.to(dt)
    n, D = z1.shape[0] * comm.world_size(), z1.shape[1]
    d = z1 - z2
    sums = comm.all_reduce_with_grad(torch.stack([z1.sum(0), z2.sum(0), (d * d).sum(0)]))
    x1, x2 = z1 - sums[0] / n, z2 - sums[1] / n
    C = comm.all_reduce_with_grad(torch.stack([x1.t() @ x1, x2.t() @ x2]) / (n - 1))
    var = torch.diagonal(C, dim1=1, dim2=2)
    l_sim = sums[2].sum() / (n * D)
    l_std = 0.5 * torch.relu(1 - torch.sqrt(var + eps)).sum() / D
    l_cov = ((C * C).sum() - (var * var).sum()) / D
    return sim * l_sim + std * l_std + cov * l_cov


class VICRegLoss(nn.Module):
    def __init__(self, sim: float = 25.0, std: float = 25.0, cov: float = 1.0, eps: float = 1e-4,
                 backend: str = "auto"):
        super().__init__()
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"backend {backend!r}")
        self.sim, self.std, self.cov = float(sim), float(std), float(cov)
        self.eps = float(eps)
        self.backend = backend
        self._warned = False

    def _use_native(self, z1: torch.Tensor, n_total: int) -> bool:
        if self.backend == "torch":
            return False
        from ..ops import _ext, vicreg
        if self.backend == "native":
            return True     # ops.vicreg raises on what it cannot take: never a silent fall-back
        if not (z1.is_cuda and z1.dtype == torch.float32 and _ext.available()):
            return False
        if not vicreg.supported(n_total, z1.shape[1]):
            if not self._warned:
                self._warned = True
                logging.warning(f"VICReg: N={n_total}, D={z1.shape[1]} is outside the native kernels' range "
                                f"(D = 64·j in [{vicreg.MIN_D}, {vicreg.MAX_D}]); using the torch loss")
            return False
        return True

    def forward(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        if feats.dim() != 2 or feats.shape[0] % 2:
            raise ValueError("`feats` must be [2·B][D]: view 1 of every sample, then view 2")
        b = feats.shape[0] // 2
        z1, z2 = feats[:b], feats[b:]
        w = comm.world_size()
        if self._use_native(z1, b * w):
            from ..ops import vicreg
            loss = vicreg.vicreg_loss(z1, z2, self.sim, self.std, self.cov, self.eps)
        else:
            loss = vicreg_reference(z1, z2, self.sim, self.std, self.cov, self.eps)
        return loss / w if w > 1 else loss
