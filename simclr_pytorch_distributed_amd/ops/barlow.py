"""Barlow Twins loss on the native gfx950 kernels (csrc/kernels/barlow.hip).

``barlow_loss(z1, z2, lambd, eps)`` is the differentiable loss of the GLOBAL batch (the same
value on every rank). Forward: column statistics, the MFMA cross-correlation C = ẑ1ᵀẑ2 / N, then
one pass that turns C into G = ∂L/∂C and yields the loss and the two BatchNorm-backward vectors
r1, r2. Backward: one launch, dz_v = rstd_v ⊙ (ẑ_other·G^(ᵀ)/N − ẑ_v ⊙ r_v)·g. With several ranks
the raw column sums and C are summed over the process group between the stage ops and the
upstream gradient in the backward; everything else is local. No host synchronisation.
"""
from __future__ import annotations

import torch

from ..parallel import comm
from . import _ext
from .twoview import MAX_D, MIN_D, check_views, supported  # noqa: F401


class _BarlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, lambd, eps):
        m = _ext.require()
        w = comm.world_size()
        z1, z2 = z1.contiguous(), z2.contiguous()
        if w == 1:
            n_total = 0
            loss, G, stats, r = m.barlow_fwd(z1, z2, lambd, eps)
        else:
            n_total = z1.shape[0] * w
            sums = m.barlow_colstats(z1, z2, eps, False, 0)[0]
            comm.all_reduce_sum_(sums)
            stats = m.barlow_stats_finalize(sums, n_total, eps)
            C = m.barlow_xcorr(z1, z2, stats, n_total)
            comm.all_reduce_sum_(C)
            loss, G, r = m.barlow_loss_grad(C, lambd, n_total)
        ctx.save_for_backward(z1, z2, G, stats, r)
        ctx.n_total = n_total
        return loss

    @staticmethod
    def backward(ctx, g):
        z1, z2, G, stats, r = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).clone()
        if ctx.n_total:
            comm.all_reduce_sum_(g)
        dz1, dz2 = _ext.require().barlow_bwd(z1, z2, G, stats, r, g, ctx.n_total)
        return dz1, dz2, None, None


def barlow_loss(z1: torch.Tensor, z2: torch.Tensor, lambd: float, eps: float = 1e-5) -> torch.Tensor:
    """Native Barlow Twins loss of fp32 GPU views ``[n][D]``; raises outside :func:`supported`."""
    check_views("Barlow Twins", z1, z2)
    return _BarlowLoss.apply(z1, z2, float(lambd), float(eps))
