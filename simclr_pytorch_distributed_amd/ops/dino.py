"""DINO loss on the native gfx950 kernels (csrc/kernels/dino.hip).

``dino_loss(zs, zt, vs, vt, center, temp_s, temp_t)`` is the differentiable cross-entropy between the
teacher's centred softmax and the student's, for this rank's student rows ``zs`` ``[2n][D]`` (the two
views stacked), teacher rows ``zt`` (no gradient), the student's unnormalised prototype weights ``vs``
``[K][D]`` and the teacher's ``vt``. Teacher row (v, i) goes with student row (1 − v, i). It returns this
rank's rows' sum divided by twice the GLOBAL batch, so the sum over ranks is the loss, and Σ_i ẑ_t,i of this
rank as an fp64 D-vector, from which ``center_update`` forms the new centre. Neither ``[2n][K]`` logit
matrix is written to memory. No host synchronisation anywhere.
"""
from __future__ import annotations

import torch

from ..parallel import comm
from . import _ext

MIN_D, MAX_D = 64, 256
MIN_K, MAX_K = 64, 131072


def _cut(tiles: int, blocks: int, min_span: int) -> int:
    s = max(1, min(-(-512 // blocks), tiles // min_span))
    return -(-tiles // -(-tiles // s))


def splits(n: int, D: int, K: int):
    """(prototype spans of the row sweeps, sample spans of the prototype sweep): csrc/include/dino_plan.h,
    functions of the shape alone. ``n``: samples per view."""
    tk = 32 if D <= 128 else 16
    rp = 2 * 64 * -(-n // 64)
    k_splits = _cut(K // tk, rp // 64, 3)
    r_splits = 1 if K // 64 >= 64 else _cut(rp // tk, K // 64, 2)
    return k_splits, r_splits


def supported(n: int, D: int, K: int = MIN_K) -> bool:
    """Shapes the native kernels take (dino_plan.h): n >= 1 samples per view, D = 64·j <= 256, K = 64·j in
    [64, 131072], index products below 2^31."""
    if not (n >= 1 and D % 64 == 0 and MIN_D <= D <= MAX_D and K % 64 == 0 and MIN_K <= K <= MAX_K):
        return False
    rp = 2 * 64 * -(-n // 64)
    if rp * D >= 2 ** 31:
        return False
    ks, rs = splits(n, D, K)
    return ks * rp * D < 2 ** 31 and (rs == 1 or rs * K * D < 2 ** 31)


class _DinoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, zs, zt, vs, vt, center, temp_s, temp_t, frozen):
        m = _ext.require()
        n_total = zs.shape[0] // 2 * comm.world_size()
        zs, vs = zs.contiguous(), vs.contiguous()
        loss, lse_s, lse_t, zs_pl, zt_pl, cs_pl, ct_pl, rzs, rvs, zsum = m.dino_fwd(
            zs, zt.detach().contiguous(), vs, vt.detach().contiguous(), center, temp_s, temp_t, n_total)
        ctx.save_for_backward(zs, vs, zs_pl, zt_pl, cs_pl, ct_pl, rzs, rvs, center, lse_s, lse_t)
        ctx.args = (temp_s, temp_t, n_total, frozen)
        ctx.mark_non_differentiable(zsum)
        return loss.reshape(()), zsum

    @staticmethod
    def backward(ctx, g, _gz):
        temp_s, temp_t, n_total, frozen = ctx.args
        g = g.to(torch.float32).reshape(1).contiguous()
        want_dv = ctx.needs_input_grad[2] and not frozen
        dz, dv = _ext.require().dino_bwd(*ctx.saved_tensors, g, temp_s, temp_t, n_total, want_dv)
        if not ctx.needs_input_grad[2]:
            dv = None
        elif frozen:
            dv = torch.zeros_like(ctx.saved_tensors[1])
        return dz, None, dv, None, None, None, None, None


def dino_loss(zs: torch.Tensor, zt: torch.Tensor, vs: torch.Tensor, vt: torch.Tensor, center: torch.Tensor,
              temp_s: float = 0.1, temp_t: float = 0.04, frozen: bool = False):
    """-> (loss, Σ_i ẑ_t,i of this rank as fp64 ``[D]``); raises outside :func:`supported`. With ``frozen``
    the prototypes' gradient is zero and their sweep is not launched."""
    ok = all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 for t in (zs, zt, vs, vt))
    if not (ok and zs.shape == zt.shape and vs.shape == vt.shape and zs.shape[0] % 2 == 0 and zs.shape[1] == vs.shape[1]
            and center.is_cuda and center.dtype == torch.float32 and center.numel() == vs.shape[0]
            and center.is_contiguous()):
        raise RuntimeError("DINO native backend needs fp32 GPU tensors: rows zs, zt [2n][D], prototypes vs, vt [K][D] "
                           "and a contiguous center of K elements")
    n, D, K = zs.shape[0] // 2, zs.shape[1], vs.shape[0]
    if not supported(n, D, K):
        raise RuntimeError(f"DINO native backend: unsupported shape n={n}, D={D}, K={K} (D = 64·j in [{MIN_D}, "
                           f"{MAX_D}], K = 64·j in [{MIN_K}, {MAX_K}])")
    return _DinoLoss.apply(zs, zt, vs, vt, center, float(temp_s), float(temp_t), bool(frozen))


def center_update(vt: torch.Tensor, zsum: torch.Tensor, center: torch.Tensor, m: float, rows_total: int) -> torch.Tensor:
    """m·center + (1 − m)·(column mean of the teacher logits over ``rows_total`` rows), ``zsum`` = Σ ẑ_t over
    every rank's rows: one fp64 dot per prototype."""
    return _ext.require().dino_center(vt.detach().contiguous(), zsum, center, float(m), int(rows_total))
