"""VICReg loss on the native gfx950 kernels (csrc/kernels/vicreg.hip).

``vicreg_loss(z1, z2, sim, std, cov, eps)`` is the differentiable loss of the GLOBAL batch (the same
value on every rank). Forward: column sums (the invariance term rides in their third row), the two
symmetric MFMA covariances C_v = x̄_vᵀx̄_v / (N − 1), then one pass that turns C into G (the
off-diagonal gradient, scaled) and yields the loss, its three terms and the hinge coefficients.
Backward: one launch, dz_v = g·(x̄_v·G_v − coef_v ⊙ x̄_v + 2λ/(N·D)·(z_v − z_other)). With several
ranks the raw column sums and C are summed over the process group between the stage ops and the
upstream gradient in the backward; everything else is local. No host synchronisation.
"""
from __future__ import annotations

import torch

from ..parallel import comm
from . import _ext
from .twoview import MAX_D, MIN_D, check_views, supported  # noqa: F401


class _VICRegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, sim, std, cov, eps):
        m = _ext.require()
        w = comm.world_size()
        z1, z2 = z1.contiguous(), z2.contiguous()
        if w == 1:
            n_total = 0
            loss, terms, G, mu, coef = m.vicreg_fwd(z1, z2, sim, std, cov, eps)
        else:
            n_total = z1.shape[0] * w
            sums = m.vicreg_colstats(z1, z2, False, 0)[0]
            comm.all_reduce_sum_(sums)
            mu = m.vicreg_stats_finalize(sums, n_total)
            C = m.vicreg_cov(z1, z2, mu, n_total)
            comm.all_reduce_sum_(C)
            loss, terms, G, coef = m.vicreg_loss_grad(C, sums, sim, std, cov, eps, n_total)
        ctx.save_for_backward(z1, z2, G, mu, coef)
        ctx.n_total, ctx.sim = n_total, sim
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        z1, z2, G, mu, coef = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).clone()
        if ctx.n_total:
            comm.all_reduce_sum_(g)
        dz1, dz2 = _ext.require().vicreg_bwd(z1, z2, G, mu, coef, g, ctx.sim, ctx.n_total)
        return dz1, dz2, None, None, None, None


def vicreg_loss(z1: torch.Tensor, z2: torch.Tensor, sim: float = 25.0, std: float = 25.0, cov: float = 1.0,
                eps: float = 1e-4) -> torch.Tensor:
    """Native VICReg loss of fp32 GPU views ``[n][D]``; raises outside :func:`supported`."""
    check_views("VICReg", z1, z2)
    return _VICRegLoss.apply(z1, z2, float(sim), float(std), float(cov), float(eps))
