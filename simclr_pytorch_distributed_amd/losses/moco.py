"""MoCo v2 loss (He et al., 2020; Chen et al., 2020), the asymmetric form of the official
``moco/builder.py``: queries from the trained encoder, keys from its momentum copy, and a ring buffer of
the K most recent keys as negatives.

For q̂ = q / ‖q‖, k̂ = k / ‖k‖ row-wise and the queue rows Q_j:

    l⁺_i = q̂_i·k̂_i          l⁻_ij = q̂_i·Q_j          (T = 0.2)
    L = −1/N·Σ_i [l⁺_i/T − log(exp(l⁺_i/T) + Σ_j exp(l⁻_ij/T))]

which is ``cross_entropy(cat([l⁺, l⁻], 1) / T, 0)``. No gradient reaches k or the queue. After the loss
the keys of the global batch overwrite slots (ptr + i) mod K and ptr advances by N.

The queue is stored on every backend as two bf16 planes ``[2][K][D]``, hi = bf16(x) and lo = bf16(x − hi),
and its value is DEFINED as hi + lo: the planes are the native kernels' MFMA operands as they lie in
memory, and a checkpoint means the same on either backend.

* :func:`moco_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch`` and the
  oracle's twin.
* :class:`MoCoLoss` — the criterion; on the GPU it runs the native kernels (ops/moco.py).

With W ranks N is the global batch: each rank returns its own rows' sum over N, so the sum over ranks is
L (the convention of losses/twoview.py), and ``enqueue`` all-gathers the keys without gradient.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import moco
from ..parallel import comm


def queue_value(queue: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """The rows ``[K][D]`` that the planes ``[2][K][D]`` stand for."""
    return queue[0].to(dtype) + queue[1].to(dtype)


def moco_reference(q: torch.Tensor, k: torch.Tensor, queue: torch.Tensor, temp: float = 0.2) -> torch.Tensor:
    """This rank's rows' sum over the global batch (differentiable in q). ``queue``: the planes
    ``[2][K][D]`` or the rows ``[K][D]`` themselves."""
    dt = torch.promote_types(q.dtype, torch.float32)
    n = q.shape[0] * comm.world_size()
    qh = F.normalize(q.to(dt), dim=1)
    with torch.no_grad():
        kh = F.normalize(k.to(dt), dim=1)
        Q = queue_value(queue, dt) if queue.dim() == 3 else queue.to(dt)
    logits = torch.cat([(qh * kh).sum(1, keepdim=True), qh @ Q.t()], dim=1) / temp
    return (torch.logsumexp(logits, dim=1) - logits[:, 0]).sum() / n


class MoCoLoss(nn.Module):
    """Owns the ring buffer: ``queue`` (bf16 planes ``[2][K][D]``) and ``ptr`` (one int64), both
    buffers on the module's device. ``forward(q, k)`` is the loss; ``enqueue(k)`` follows the step.
    A fresh queue holds row-normalised Gaussian rows drawn from ``seed``. ``backend="native"`` raises
    when the kernels cannot take the call; ``"auto"`` uses the twin then, and warns once."""

    def __init__(self, K: int = 65536, D: int = 128, temp: float = 0.2, backend: str = "auto", seed: int = 0):
        super().__init__()
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"backend {backend!r}")
        if K < 1 or D < 1 or not temp > 0:
            raise ValueError("K >= 1, D >= 1 and temp > 0 are required")
        self.K, self.D, self.temp, self.backend = int(K), int(D), float(temp), backend
        gen = torch.Generator().manual_seed(int(seed))
        rows = F.normalize(torch.randn(self.K, self.D, generator=gen), dim=1)
        self.register_buffer("queue", moco.split_planes(rows))
        self.register_buffer("ptr", torch.zeros(1, dtype=torch.int64))
        self._warned = False
        self._keys = None     # (k, k̂) of the last forward: enqueue(k) does not normalise again

    def _use_native(self, q: torch.Tensor) -> bool:
        if self.backend == "torch":
            return False
        if self.backend == "native":
            return True     # the ops module raises on what it cannot take: never a silent fall-back
        from ..ops import _ext
        if not (q.is_cuda and q.dtype == torch.float32 and self.queue.is_cuda and _ext.available()):
            return False
        if not moco.supported(q.shape[0], q.shape[1], self.K):
            if not self._warned:
                self._warned = True
                logging.warning(f"MoCo: n={q.shape[0]}, D={q.shape[1]}, K={self.K} is outside the native kernels' "
                                f"range (D = 64·j in [{moco.MIN_D}, {moco.MAX_D}], K = 64·j in [{moco.MIN_K}, "
                                f"{moco.MAX_K}]); using the torch loss")
            return False
        return True

    def forward(self, q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
        if q.dim() != 2 or q.shape != k.shape or q.shape[1] != self.D:
            raise ValueError(f"q and k must be [N][{self.D}] of equal shape")
        kd = k.detach()
        if self._use_native(q):
            loss, kh = moco.moco_loss_keys(q, kd, self.queue, self.temp)
        else:
            loss = moco_reference(q, kd, self.queue, self.temp)
            kh = F.normalize(kd.to(torch.float32), dim=1)
        self._keys = (k, kh.detach())     # the caller's own tensor: enqueue(k) tests identity against it
        return loss

    @torch.no_grad()
    def enqueue(self, k: torch.Tensor) -> None:
        """The globally gathered normalised keys overwrite slots (ptr + i) mod K; ptr += N mod K.
        Given the very tensor the last ``forward`` took, the k̂ formed there (on the native path by
        ``moco_prep``: the rows the loss used) is enqueued; any other tensor is normalised here. Call
        it AFTER ``backward()``: the loss's graph holds the queue, and the enqueue bumps the queue's
        version, so a backward through an earlier loss then raises instead of using the new rows."""
        cached = self._keys is not None and self._keys[0] is k
        kh = self._keys[1] if cached else F.normalize(k.detach().to(torch.float32), dim=1)
        self._keys = None
        keys = comm.all_gather_tensor(kh)
        n = keys.shape[0]
        if n > self.K:
            raise ValueError(f"{n} keys do not fit a queue of {self.K}")
        from ..ops import _ext
        fits = keys.is_cuda and self.queue.is_cuda and moco.supported(1, self.D, self.K)
        if self.backend == "native" and not fits:
            raise RuntimeError(f"MoCo native backend: cannot enqueue D={self.D}, K={self.K} on {keys.device.type}")
        if self.backend == "native" or (self.backend == "auto" and fits and _ext.available()):
            moco.enqueue(self.queue, self.ptr, keys)
            return
        slots = (self.ptr + torch.arange(n, device=self.ptr.device)) % self.K
        self.queue[:, slots] = moco.split_planes(keys).to(self.queue.device)
        self.ptr.copy_((self.ptr + n) % self.K)
