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
* :class:`VICRegLoss` — the criterion (losses/twoview.py); on the GPU it runs the native kernels
  (ops/vicreg.py).

With W ranks N is the global batch: the column sums, the invariance sum and C are summed over the
process group (differentiably in the twin).
"""
from __future__ import annotations

import torch

from ..ops import vicreg
from ..parallel import comm
from .twoview import TwoViewLoss


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


class VICRegLoss(TwoViewLoss):
    name, ops = "VICReg", vicreg

    def __init__(self, sim: float = 25.0, std: float = 25.0, cov: float = 1.0, eps: float = 1e-4,
                 backend: str = "auto"):
        super().__init__(backend)
        self.sim, self.std, self.cov = float(sim), float(std), float(cov)
        self.eps = float(eps)

    def native(self, z1, z2):
        return vicreg.vicreg_loss(z1, z2, self.sim, self.std, self.cov, self.eps)

    def twin(self, z1, z2):
        return vicreg_reference(z1, z2, self.sim, self.std, self.cov, self.eps)
