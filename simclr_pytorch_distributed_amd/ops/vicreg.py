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

MIN_D, MAX_D = 64, 8192


def supported(n: int, D: int) -> bool:
    """Shapes the native kernels take: D = 64·j in [64, 8192], at least 2 rows, n·D < 2^31."""
    return D % 64 == 0 and MIN_D <= D <= MAX_D and n >= 2 and n * D < 2 ** 31


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
    if not (z1.is_cuda and z1.dtype == torch.float32 and z2.dtype == torch.float32 and z1.shape == z2.shape
            and z1.dim() == 2):
        raise RuntimeError("VICReg native backend needs two fp32 GPU tensors [n][D] of equal shape")
    n, D = z1.shape[0] * comm.world_size(), z1.shape[1]
    if not supported(n, D):
        raise RuntimeError(f"VICReg native backend: unsupported shape N={n}, D={D} "
                           f"(D = 64·j in [{MIN_D}, {MAX_D}], N >= 2)")
    return _VICRegLoss.apply(z1, z2, float(sim), float(std), float(cov), float(eps))
