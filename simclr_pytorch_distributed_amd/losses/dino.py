"""DINO loss (Caron et al., 2021), the official ``DINOLoss`` / ``DINOHead`` restricted to two global crops:
self-distillation from a momentum teacher onto K prototypes.

For the row-normalised projector outputs ẑ_s, ẑ_t ``[2N][D]`` (the two views stacked) and the row-normalised
prototype weights Ĉ_s, Ĉ_t ``[K][D]`` (``weight_norm`` with g ≡ 1, ``norm_last_layer=True``):

    s = ẑ_s·Ĉ_sᵀ          t = ẑ_t·Ĉ_tᵀ
    p_t(v,i,·) = softmax((t(v,i,·) − c)/τ_t)                                        (no gradient)
    L = 1/(2N)·Σ_v Σ_i [lse(s(1−v,i,·)/τ_s) − Σ_k p_t(v,i,k)·s(1−v,i,k)/τ_s]
    c ← m_c·c + (1 − m_c)·mean over all 2N teacher rows of t                        (after the loss)

The gradient reaches the student's rows and the student's UNNORMALISED weights V_s, through both
normalisations. The centre's update needs no second pass over t: its column mean is Ĉ_t·(Σ_i ẑ_t,i)/(2N).

* :func:`dino_reference`, :func:`center_reference` — plain torch, any device and dtype: the CPU path,
  ``--backend torch`` and the oracle's twin.
* :class:`DINOLoss` — the criterion; on the GPU it runs the native kernels (ops/dino.py).

With W ranks N is the global batch: each rank returns its own rows' sum over 2N, so the sum over ranks is L
(the convention of losses/twoview.py); the only extra collective is the all-reduce of the D-vector Σ_i ẑ_t.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import dino
from ..parallel import comm


def dino_reference(zs: torch.Tensor, zt: torch.Tensor, vs: torch.Tensor, vt: torch.Tensor, center: torch.Tensor,
                   temp_s: float = 0.1, temp_t: float = 0.04) -> torch.Tensor:
    """This rank's rows' sum over twice the global batch (differentiable in zs and vs)."""
    dt = torch.promote_types(zs.dtype, torch.float32)
    n = zs.shape[0] // 2
    s = F.normalize(zs.to(dt), dim=1) @ F.normalize(vs.to(dt), dim=1).t()
    with torch.no_grad():
        t = F.normalize(zt.to(dt), dim=1) @ F.normalize(vt.to(dt), dim=1).t()
        pt = torch.softmax((t - center.to(dt)) / temp_t, dim=1)
        pt = torch.cat([pt[n:], pt[:n]])     # teacher view v goes with student view 1 − v
    return -(pt * torch.log_softmax(s / temp_s, dim=1)).sum() / (2 * n * comm.world_size())


def teacher_sum(zt: torch.Tensor) -> torch.Tensor:
    """Σ_i ẑ_t,i of this rank's rows in fp64: what the centre's update needs of the batch."""
    return F.normalize(zt.detach().to(torch.float64), dim=1).sum(0)


def center_reference(zsum: torch.Tensor, vt: torch.Tensor, center: torch.Tensor, m: float, rows_total: int) -> torch.Tensor:
    """m·c + (1 − m)·Ĉ_t·zsum/rows_total, ``zsum`` summed over every rank."""
    mean = F.normalize(vt.detach().to(torch.float64), dim=1) @ zsum.to(torch.float64) / rows_total
    return (m * center.to(torch.float64) + (1 - m) * mean).to(center.dtype)


class DINOLoss(nn.Module):
    """Owns the ``center`` buffer ``[K]``. ``forward(zs, zt, vs, vt)`` is the loss of the stacked views
    against the student's and the teacher's prototype weights; ``update_center()`` follows ``backward()``.
    ``temps`` = (τ_s, τ_t); the teacher's schedule is the caller's (:meth:`set_teacher_temp`). While
    :meth:`set_frozen` is on, the prototypes' gradient is zero. ``backend="native"`` raises when the
    kernels cannot take the call; ``"auto"`` uses the twin then, and warns once."""

    def __init__(self, K: int = 65536, temps=(0.1, 0.04), center_momentum: float = 0.9, backend: str = "auto"):
        super().__init__()
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"backend {backend!r}")
        ts, tt = (float(x) for x in temps)
        if K < 1 or not (ts > 0 and tt > 0) or not 0.0 <= center_momentum <= 1.0:
            raise ValueError("K >= 1, temperatures > 0 and 0 <= center_momentum <= 1 are required")
        self.K, self.temp_s, self.temp_t, self.center_momentum, self.backend = int(K), ts, tt, float(center_momentum), backend
        self.register_buffer("center", torch.zeros(self.K))
        self.frozen = False
        self._warned = False
        self._pending = None     # (Σ ẑ_t of this rank, the teacher's weights, rows on this rank, native?)

    def set_teacher_temp(self, temp_t: float) -> None:
        self.temp_t = float(temp_t)

    def set_frozen(self, frozen: bool) -> None:
        self.frozen = bool(frozen)

    def _use_native(self, zs: torch.Tensor, vs: torch.Tensor) -> bool:
        if self.backend == "torch":
            return False
        if self.backend == "native":
            return True     # the ops module raises on what it cannot take: never a silent fall-back
        from ..ops import _ext
        if not (zs.is_cuda and zs.dtype == torch.float32 and vs.is_cuda and vs.dtype == torch.float32
                and self.center.is_cuda and _ext.available()):
            return False
        if not dino.supported(zs.shape[0] // 2, zs.shape[1], self.K):
            if not self._warned:
                self._warned = True
                logging.warning(f"DINO: n={zs.shape[0] // 2}, D={zs.shape[1]}, K={self.K} is outside the native kernels' "
                                f"range (D = 64·j in [{dino.MIN_D}, {dino.MAX_D}], K = 64·j in [{dino.MIN_K}, "
                                f"{dino.MAX_K}]); using the torch loss")
            return False
        return True

    def forward(self, zs: torch.Tensor, zt: torch.Tensor, vs: torch.Tensor, vt: torch.Tensor) -> torch.Tensor:
        if zs.dim() != 2 or zs.shape != zt.shape or zs.shape[0] % 2 or vs.shape != vt.shape \
                or tuple(vs.shape) != (self.K, zs.shape[1]):
            raise ValueError(f"zs and zt must be [2N][D] of equal shape, vs and vt [{self.K}][D]")
        zt, vt = zt.detach(), vt.detach()
        native = self._use_native(zs, vs)
        if native:
            loss, zsum = dino.dino_loss(zs, zt, vs, vt, self.center, self.temp_s, self.temp_t, self.frozen)
        else:
            loss = dino_reference(zs, zt, vs.detach() if self.frozen else vs, vt, self.center, self.temp_s, self.temp_t)
            zsum = teacher_sum(zt)
        self._pending = (zsum, vt, zs.shape[0], native)
        return loss

    @torch.no_grad()
    def update_center(self) -> None:
        """c ← m_c·c + (1 − m_c)·(column mean of the last forward's teacher logits over every rank's rows).
        Call it AFTER ``backward()``: the loss's graph holds the centre."""
        if self._pending is None:
            raise RuntimeError("update_center() follows a forward()")
        zsum, vt, rows, native = self._pending
        self._pending = None
        if comm.world_size() > 1:
            zsum = comm.all_reduce_sum_(zsum.clone())
        rows_total = rows * comm.world_size()
        if native:
            new = dino.center_update(vt, zsum, self.center, self.center_momentum, rows_total)
        else:
            new = center_reference(zsum, vt, self.center, self.center_momentum, rows_total)
        self.center.copy_(new)
