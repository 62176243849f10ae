"""MoCo loss on the native gfx950 kernels (csrc/kernels/moco.hip).

``moco_loss(q, k, queue, temp)`` is the differentiable InfoNCE of this rank's queries ``q`` ``[n][D]``
against their keys ``k`` (no gradient) and the K negatives of ``queue``, a bf16 tensor ``[2][K][D]`` whose
value is plane 0 + plane 1 (hi = bf16(x), lo = bf16(x − hi)). It returns this rank's rows' sum divided by
the GLOBAL batch, so the sum over ranks is the loss. ``enqueue`` overwrites ring-buffer slots and advances
the device-resident pointer; ``ema_update`` is the momentum encoder's step over flat fp32 buffers. No
host synchronisation anywhere.
"""
from __future__ import annotations

import torch

from ..parallel import comm
from . import _ext

MIN_D, MAX_D = 64, 256
MIN_K, MAX_K = 64, 1 << 20


def supported(n: int, D: int, K: int = MIN_K) -> bool:
    """Shapes the native kernels take (csrc/include/moco_plan.h): n >= 1 query rows, D = 64·j <= 256,
    K = 64·j in [64, 2^20], index products below 2^31."""
    if not (n >= 1 and D % 64 == 0 and MIN_D <= D <= MAX_D and K % 64 == 0 and MIN_K <= K <= MAX_K):
        return False
    return K * D < 2 ** 31 and splits(n, K) * n * D < 2 ** 31


def splits(n: int, K: int) -> int:
    """Workgroups along the queue axis (moco_plan.h): a function of (n, K) alone."""
    tiles = K // 32
    s = max(1, min(-(-512 // -(-n // 64)), tiles // 3))
    return -(-tiles // -(-tiles // s))


def split_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows ``[R][D]`` -> the two bf16 planes ``[2][R][D]`` (any device)."""
    x = x.to(torch.float32)
    hi = x.to(torch.bfloat16)
    return torch.stack([hi, (x - hi.to(torch.float32)).to(torch.bfloat16)])


class _MoCoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, queue, temp):
        m = _ext.require()
        n_total = q.shape[0] * comm.world_size()
        loss, lse, lpos, qhat, rq, khat = m.moco_fwd(q.contiguous(), k.detach().contiguous(), queue, temp, n_total)
        ctx.save_for_backward(qhat, rq, khat, queue, lse, lpos)
        ctx.temp, ctx.n_total = temp, n_total
        ctx.mark_non_differentiable(khat)
        return loss.reshape(()), khat

    @staticmethod
    def backward(ctx, g, _gk):
        qhat, rq, khat, queue, lse, lpos = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()
        dq, _ = _ext.require().moco_bwd(qhat, rq, khat, queue, lse, lpos, g, ctx.temp, ctx.n_total)
        return dq, None, None, None


def moco_loss(q: torch.Tensor, k: torch.Tensor, queue: torch.Tensor, temp: float = 0.2) -> torch.Tensor:
    """Native MoCo loss of fp32 GPU rows ``[n][D]`` and a bf16 queue ``[2][K][D]``; raises outside
    :func:`supported`."""
    return moco_loss_keys(q, k, queue, temp)[0]


def moco_loss_keys(q: torch.Tensor, k: torch.Tensor, queue: torch.Tensor, temp: float = 0.2):
    """:func:`moco_loss` and the normalised keys k̂ ``[n][D]`` the kernels formed (what ``enqueue`` takes)."""
    if not (q.is_cuda and q.dtype == torch.float32 and k.dtype == torch.float32 and q.dim() == 2
            and q.shape == k.shape and queue.is_cuda and queue.dtype == torch.bfloat16 and queue.dim() == 3
            and queue.shape[0] == 2 and queue.shape[2] == q.shape[1] and queue.is_contiguous()):
        raise RuntimeError("MoCo native backend needs fp32 GPU tensors q, k [n][D] of equal shape and a contiguous "
                           "bf16 GPU queue [2][K][D]")
    n, D, K = q.shape[0], q.shape[1], queue.shape[1]
    if not supported(n, D, K):
        raise RuntimeError(f"MoCo native backend: unsupported shape n={n}, D={D}, K={K} (D = 64·j in [{MIN_D}, "
                           f"{MAX_D}], K = 64·j in [{MIN_K}, {MAX_K}])")
    return _MoCoLoss.apply(q, k, queue, float(temp))


def enqueue(queue: torch.Tensor, ptr: torch.Tensor, keys: torch.Tensor) -> None:
    """``keys`` ``[n][D]`` (normalised fp32 rows, n <= K) into slots (ptr + i) mod K; ptr += n mod K."""
    _ext.require().moco_enqueue(queue, ptr, keys.detach().contiguous())
    # the op writes through raw pointers: tell autograd, so a graph that saved the queue notices
    torch.autograd.graph.increment_version(queue)
    torch.autograd.graph.increment_version(ptr)


def ema_update(dst: torch.Tensor, src: torch.Tensor, m: float) -> None:
    """dst <- m·dst + (1 − m)·src in place, two flat fp32 GPU buffers of equal length."""
    _ext.require().ema_update(dst, src, float(m))
