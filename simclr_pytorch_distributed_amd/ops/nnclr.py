"""NNCLR loss on the native gfx950 kernels (csrc/kernels/nnclr.hip).

``nn_search(z, queue)`` is the top-1 search of row-normalised ``z`` in the support queue, a bf16 tensor
``[2][K][D]`` whose value is plane 0 + plane 1 (MoCo's format, ``ops.moco.split_planes``); ties go to the
lower queue index. ``nnclr_loss(z, p, queue, temp)`` is the cross-view InfoNCE of the neighbours of this
rank's projections ``z`` ``[2n][D]`` (view-major, no gradient) against the predictions ``p``, differentiable
in the predictions alone. It returns this rank's rows' sum divided by the GLOBAL 2N, so the sum over ranks
is the loss. The enqueue is ``ops.moco.enqueue``. No host synchronisation anywhere.
"""
from __future__ import annotations

import torch

from . import _ext

MIN_D, MAX_D = 64, 256
MIN_K, MAX_K = 64, 1 << 20


def _cut(blocks: int, tiles: int) -> tuple:
    """(splits, tiles of a span) of a streamed axis (nnclr_plan.h ``cut``)."""
    s = max(1, min(-(-512 // blocks), tiles // 3))
    span = -(-tiles // s)
    return -(-tiles // span), span


def splits(n: int, K: int) -> int:
    """Workgroups along the queue axis of the search (nnclr_plan.h): a function of (n, K) alone."""
    return _cut(-(-2 * n // 64), K // 32)[0]


def span(n: int, K: int) -> int:
    """Queue rows of one search split: split s covers rows [s·span, min(K, (s + 1)·span))."""
    return 32 * _cut(-(-2 * n // 64), K // 32)[1]


def supported(n: int, D: int, K: int = MIN_K, N: int = 0) -> bool:
    """Shapes the native kernels take (csrc/include/nnclr_plan.h): n >= 1 rows per view on this rank,
    N >= n per view in the global batch, D = 64·j <= 256, K = 64·j in [64, 2^20], index products below 2^31."""
    N = N or n
    if not (1 <= n <= N and D % 64 == 0 and MIN_D <= D <= MAX_D and K % 64 == 0 and MIN_K <= K <= MAX_K):
        return False
    if 2 * N * D >= 2 ** 31 or K * D >= 2 ** 31:
        return False
    fwd = _cut(2 * -(-n // 64), -(-N // 32))[0]
    bwd = _cut(2 * -(-N // 64), -(-n // 32))[0]
    return max(splits(n, K) * 4 * n, fwd * 4 * n, bwd * 2 * N * D) < 2 ** 31


def _check_queue(x: torch.Tensor, queue: torch.Tensor) -> None:
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] % 2 == 0 and x.shape[0] >= 2
            and queue.is_cuda and queue.dtype == torch.bfloat16 and queue.dim() == 3 and queue.shape[0] == 2
            and queue.shape[2] == x.shape[1] and queue.is_contiguous()):
        raise RuntimeError("NNCLR native backend needs fp32 GPU rows [2n][D] (view-major) and a contiguous bf16 GPU "
                           "queue [2][K][D]")


def _check_shape(n: int, D: int, K: int, N: int) -> None:
    if not supported(n, D, K, N):
        raise RuntimeError(f"NNCLR native backend: unsupported shape n={n}, N={N}, D={D}, K={K} (D = 64·j in "
                           f"[{MIN_D}, {MAX_D}], K = 64·j in [{MIN_K}, {MAX_K}])")


@torch.no_grad()
def nn_search(z: torch.Tensor, queue: torch.Tensor):
    """(idx int32 ``[2n]``, similarity ``[2n]``) of the nearest queue row of every row of ``z`` ``[2n][D]``
    (normalised here); raises outside :func:`supported`."""
    _check_queue(z, queue)
    _check_shape(z.shape[0] // 2, z.shape[1], queue.shape[1], 0)
    m = _ext.require()
    idx, sim, _ = m.nnclr_search(m.nnclr_prep(z.detach().contiguous())[1], queue)
    return idx, sim


class _NNCLRLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, p_all, queue, temp, pos_offset):
        m = _ext.require()
        p2 = p_all.contiguous().view(-1, p_all.shape[-1])
        loss, lse, idx, _sim, zhat, nnpl, ppl, rp = m.nnclr_fwd(z.detach().contiguous(), p2, queue, temp, pos_offset)
        ctx.save_for_backward(nnpl, ppl, p2, rp, lse, queue)     # the queue: a later enqueue is then noticed
        ctx.temp, ctx.pos_offset, ctx.shape = temp, pos_offset, p_all.shape
        ctx.mark_non_differentiable(zhat, idx)
        return loss.reshape(()), zhat, idx

    @staticmethod
    def backward(ctx, g, _gz, _gi):
        nnpl, ppl, p2, rp, lse, _queue = ctx.saved_tensors
        g = g.to(torch.float32).reshape(1).contiguous()
        dp, _ = _ext.require().nnclr_bwd(nnpl, ppl, p2, rp, lse, g, ctx.temp, ctx.pos_offset)
        return None, dp.view(ctx.shape), None, None, None


def nnclr_loss_rows(z: torch.Tensor, p: torch.Tensor, queue: torch.Tensor, temp: float = 0.1, pos_offset: int = 0,
                    p_all: torch.Tensor = None):
    """:func:`nnclr_loss`, the normalised projections ẑ ``[2n][D]`` the kernels formed (view 1's are what the
    enqueue takes) and the neighbours' queue indices (int32 ``[2n]``)."""
    _check_queue(z, queue)
    n, D = z.shape[0] // 2, z.shape[1]
    rows = p.reshape(2, n, D) if p_all is None else p_all
    if not (rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 3 and rows.shape[0] == 2
            and rows.shape[2] == D and 0 <= pos_offset <= rows.shape[1] - n):
        raise RuntimeError("NNCLR native backend needs fp32 GPU predictions [2n][D], or gathered ones [2][N][D] with "
                           "0 <= pos_offset <= N - n")
    _check_shape(n, D, queue.shape[1], rows.shape[1])
    return _NNCLRLoss.apply(z, rows, queue, float(temp), int(pos_offset))


def nnclr_loss(z: torch.Tensor, p: torch.Tensor, queue: torch.Tensor, temp: float = 0.1, pos_offset: int = 0,
               p_all: torch.Tensor = None) -> torch.Tensor:
    """Native NNCLR loss of fp32 GPU rows ``z``, ``p`` ``[2n][D]`` (view-major) and a bf16 queue ``[2][K][D]``.
    With several ranks ``p_all`` is the gathered (unnormalised) ``[2][N][D]`` predictions, this rank's at rows
    ``pos_offset .. pos_offset + n`` of each view: the gradient then goes to all of ``p_all`` and ``p`` is not
    read. ``z`` receives no gradient. Raises outside :func:`supported`."""
    return nnclr_loss_rows(z, p, queue, temp, pos_offset, p_all)[0]
