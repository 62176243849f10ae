"""SwAV loss on the native gfx950 kernels (csrc/kernels/swav.hip).

``swav_loss(z1, z2, C, eps, temp, iters, freeze)`` is the differentiable two-crop SwAV loss of the
GLOBAL batch (the same value on every rank). ``C`` ``[K][D]`` is the prototype matrix; its rows are
normalised IN PLACE, without gradient, before the scores are taken. Forward: ẑ and the normalised C,
the scores S_v = ẑ_v·Cᵀ of both views (MFMA), ``iters`` Sinkhorn iterations on exp(S/ε), then one pass
that yields the loss and dS with the codes q as constants. Backward: dẑ = dS·C and dC = dSᵀ·ẑ (MFMA) and
the normalisation's backward; with ``freeze`` the dC GEMM is skipped and dC is zeros. With several
ranks the per-prototype sums r of every Sinkhorn iteration and the loss are summed over the process
group between the stage ops, and the upstream gradient in the backward; everything else is local. No
host synchronisation.
"""
from __future__ import annotations

import torch

from ..parallel import comm
from . import _ext

MIN_D, MAX_D = 64, 2048
MIN_K, MAX_K = 2, 16384


def supported(n: int, D: int, K: int = MIN_K, iters: int = 1) -> bool:
    """Shapes the native kernels take (csrc/include/swav_plan.h): n >= 2 rows per view, D = 64·j in
    [64, 2048], 2 <= K <= 16384, 2n·Kp < 2^31 with Kp = K rounded up to 64."""
    return (D % 64 == 0 and MIN_D <= D <= MAX_D and n >= 2 and MIN_K <= K <= MAX_K and iters >= 1
            and 2 * n * (-(-K // 64) * 64) < 2 ** 31)


class _SwAVLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z1, z2, C, eps, temp, iters, freeze):
        m = _ext.require()
        w = comm.world_size()
        z1, z2 = z1.contiguous(), z2.contiguous()
        Cn = C.detach()
        if w == 1:
            loss, zhat, rnorm, dS = m.swav_fwd(z1, z2, Cn, eps, temp, iters)
        else:
            n_total = z1.shape[0] * w
            zhat, rnorm = m.swav_prep(z1, z2, Cn)
            S, part = m.swav_scores(zhat, Cn, eps)
            for it in range(iters):
                r = comm.all_reduce_sum_(m.swav_rowsum(part))
                out = m.swav_sinkhorn(S, r, eps, it + 1 == iters, n_total)
                part = out[0]
            loss, dS, _ = m.swav_loss_grad(S, out[0], out[1], eps, temp, n_total)
            comm.all_reduce_sum_(loss)
        ctx.save_for_backward(zhat, rnorm, Cn, dS)
        ctx.freeze, ctx.multi = freeze, w > 1
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        zhat, rnorm, Cn, dS = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).clone()
        if ctx.multi:
            comm.all_reduce_sum_(g)
        dz, dC, _ = _ext.require().swav_bwd(zhat, rnorm, Cn, dS, g, ctx.freeze)
        n = dz.shape[0] // 2
        return dz[:n], dz[n:], dC, None, None, None, None


def swav_loss(z1: torch.Tensor, z2: torch.Tensor, C: torch.Tensor, eps: float = 0.05, temp: float = 0.1,
              iters: int = 3, freeze: bool = False) -> torch.Tensor:
    """Native SwAV loss of fp32 GPU views ``[n][D]`` and prototypes ``[K][D]`` (normalised in place);
    raises outside :func:`supported`."""
    if not (z1.is_cuda and z1.dtype == torch.float32 and z2.dtype == torch.float32 and z1.shape == z2.shape
            and z1.dim() == 2 and C.is_cuda and C.dtype == torch.float32 and C.dim() == 2
            and C.shape[1] == z1.shape[1] and C.is_contiguous()):
        raise RuntimeError("SwAV native backend needs two fp32 GPU tensors [n][D] of equal shape and contiguous "
                           "fp32 GPU prototypes [K][D]")
    n, D, K = z1.shape[0], z1.shape[1], C.shape[0]
    if not supported(n, D, K, iters):
        raise RuntimeError(f"SwAV native backend: unsupported shape n={n}, D={D}, K={K}, iters={iters} "
                           f"(D = 64·j in [{MIN_D}, {MAX_D}], K in [{MIN_K}, {MAX_K}], n >= 2)")
    return _SwAVLoss.apply(z1, z2, C, float(eps), float(temp), int(iters), bool(freeze))
