"""NNCLR loss (Dwibedi et al., 2021, "With a Little Help from My Friends"), Algorithm 1, symmetrised as
there: the positive of a view's prediction is the nearest neighbour, in a support queue, of the OTHER
view's projection.

For the projections z ``[2n][D]`` (view-major) of the one trained model, the predictions p = predictor(z),
ẑ and p̂ their row-normalised forms and the queue rows Q_j (normalised):

    idx_v[i] = argmax_j ẑ_v[i]·Q_j  (ties to the lower j)        nn_v[i] = Q[idx_v[i]]
    L = 1/(2N)·Σ_v Σ_i [lse_k(nn_v[i]·p̂_{1−v}[k]/τ) − nn_v[i]·p̂_{1−v}[i]/τ]          (τ = 0.1)

which is ``cross_entropy(nn_v @ p̂_{1−v}.T / τ, arange(N))`` averaged over the views. The search carries no
gradient and the neighbours are constants, so the gradient reaches p only (and the encoder through the
predictor). After the update the globally gathered ẑ of view 1 overwrites slots (ptr + i) mod K.

The queue is MoCo's on every backend: two bf16 planes ``[2][K][D]``, its value DEFINED as hi + lo
(losses/moco.py).

* :func:`nnclr_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch`` and the
  oracle's twin.
* :class:`NNCLRLoss` — the criterion; on the GPU it runs the native kernels (ops/nnclr.py).

With W ranks N is the global batch per view and k runs over it: a rank searches its own rows, the
predictions are all-gathered with gradient, each rank returns its own rows' sum over 2N, so the sum over
ranks is L (the convention of losses/twoview.py), and ``enqueue`` all-gathers view 1's ẑ without gradient.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import moco, nnclr
from ..parallel import comm
from .moco import queue_value


def _gather_views(p: torch.Tensor) -> torch.Tensor:
    """This rank's ``[2n][D]`` -> the global ``[2][N][D]``, rank r's rows at r·n .. (r + 1)·n of each view."""
    n = p.shape[0] // 2
    rows = p.reshape(2, n, -1)
    if comm.world_size() == 1:
        return rows
    return comm.all_gather_with_grad(rows.transpose(0, 1).contiguous()).transpose(0, 1)


def nn_index(zh: torch.Tensor, Q: torch.Tensor) -> torch.Tensor:
    """argmax_j zh_i·Q_j per row, ties to the lower j (``torch.argmax`` promises no order among equals)."""
    sim = zh @ Q.t()
    at_max = sim == sim.max(dim=1, keepdim=True).values
    return torch.where(at_max, torch.arange(Q.shape[0], device=sim.device), Q.shape[0]).min(dim=1).values


def nnclr_reference(z: torch.Tensor, p: torch.Tensor, queue: torch.Tensor, temp: float = 0.1, pos_offset: int = None,
                    p_all: torch.Tensor = None) -> torch.Tensor:
    """This rank's rows' sum over the global 2N (differentiable in p, or in ``p_all`` when the gathered
    ``[2][N][D]`` predictions are given). ``queue``: the planes ``[2][K][D]`` or the rows ``[K][D]``."""
    dt = torch.promote_types(p.dtype if p_all is None else p_all.dtype, torch.float32)
    n = z.shape[0] // 2
    if p_all is None:
        p_all = _gather_views(p)
    if pos_offset is None:
        pos_offset = comm.rank() * n
    with torch.no_grad():
        Q = queue_value(queue, dt) if queue.dim() == 3 else queue.to(dt)
        nbr = Q[nn_index(F.normalize(z.detach().to(dt), dim=1), Q)].view(2, n, -1)
    ph = F.normalize(p_all.to(dt), dim=2)
    own = pos_offset + torch.arange(n, device=ph.device)
    loss = 0.0
    for v in range(2):
        logits = nbr[v] @ ph[1 - v].t() / temp
        loss = loss + (torch.logsumexp(logits, dim=1) - logits[torch.arange(n, device=ph.device), own]).sum()
    return loss / (2 * p_all.shape[1])


class NNCLRLoss(nn.Module):
    """Owns the support queue: ``queue`` (bf16 planes ``[2][K][D]``) and ``ptr`` (one int64), both buffers on
    the module's device. ``forward(z, p)`` is the loss; ``enqueue(z)`` follows the step. A fresh queue holds
    row-normalised Gaussian rows drawn from ``seed``. ``backend="native"`` raises when the kernels cannot
    take the call; ``"auto"`` uses the twin then, and warns once."""

    def __init__(self, K: int = 98304, D: int = 128, temp: float = 0.1, backend: str = "auto", seed: int = 0):
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
        self._rows = None     # (z, ẑ of view 1) of the last forward: enqueue(z) does not normalise again

    def _use_native(self, z: torch.Tensor, p: torch.Tensor) -> bool:
        if self.backend == "torch":
            return False
        if self.backend == "native":
            return True     # the ops module raises on what it cannot take: never a silent fall-back
        from ..ops import _ext
        if not (z.is_cuda and z.dtype == torch.float32 and p.dtype == torch.float32 and self.queue.is_cuda
                and _ext.available()):
            return False
        n = z.shape[0] // 2
        if not nnclr.supported(n, z.shape[1], self.K, n * comm.world_size()):
            if not self._warned:
                self._warned = True
                logging.warning(f"NNCLR: n={n}, D={z.shape[1]}, K={self.K} is outside the native kernels' range "
                                f"(D = 64·j in [{nnclr.MIN_D}, {nnclr.MAX_D}], K = 64·j in [{nnclr.MIN_K}, "
                                f"{nnclr.MAX_K}]); using the torch loss")
            return False
        return True

    def forward(self, z: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
        if z.dim() != 2 or z.shape != p.shape or z.shape[1] != self.D or z.shape[0] % 2:
            raise ValueError(f"z and p must be [2n][{self.D}] of equal shape, view-major")
        n = z.shape[0] // 2
        zd = z.detach()
        if self._use_native(zd, p):
            p_all = _gather_views(p) if comm.world_size() > 1 else None
            loss, zh, _ = nnclr.nnclr_loss_rows(zd, p, self.queue, self.temp, comm.rank() * n, p_all)
        else:
            loss = nnclr_reference(zd, p, self.queue, self.temp)
            zh = F.normalize(zd.to(torch.float32), dim=1)
        self._rows = (z, zh.detach()[n:])     # the caller's own tensor: enqueue(z) tests identity against it
        return loss

    @torch.no_grad()
    def enqueue(self, z: torch.Tensor) -> None:
        """The globally gathered ẑ of view 1 (rows n .. 2n of ``z``) overwrite slots (ptr + i) mod K;
        ptr += N mod K. Given the very tensor the last ``forward`` took, the ẑ formed there (on the native
        path by ``nnclr_prep``: the rows the search used) is enqueued; any other tensor is normalised here.
        Call it AFTER ``backward()``: the loss's graph holds the queue, and the enqueue bumps the queue's
        version, so a backward through an earlier loss then raises instead of passing silently (the reason
        ``MoCoLoss.enqueue`` gives)."""
        cached = self._rows is not None and self._rows[0] is z
        zh = self._rows[1] if cached else F.normalize(z.detach()[z.shape[0] // 2:].to(torch.float32), dim=1)
        self._rows = None
        keys = comm.all_gather_tensor(zh.contiguous())
        n = keys.shape[0]
        if n > self.K:
            raise ValueError(f"{n} rows do not fit a queue of {self.K}")
        from ..ops import _ext
        fits = keys.is_cuda and self.queue.is_cuda and moco.supported(1, self.D, self.K)
        if self.backend == "native" and not fits:
            raise RuntimeError(f"NNCLR native backend: cannot enqueue D={self.D}, K={self.K} on {keys.device.type}")
        if self.backend == "native" or (self.backend == "auto" and fits and _ext.available()):
            moco.enqueue(self.queue, self.ptr, keys)
            return
        slots = (self.ptr + torch.arange(n, device=self.ptr.device)) % self.K
        self.queue[:, slots] = moco.split_planes(keys).to(self.queue.device)
        self.ptr.copy_((self.ptr + n) % self.K)
