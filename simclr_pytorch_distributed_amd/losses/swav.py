"""SwAV loss (Caron et al., 2020), the two-crop form: online clustering of the two views against K
trainable prototypes, each view predicting the other's Sinkhorn-Knopp code.

For the projections z1, z2 ``[N][D]``, ẑ = z / ‖z‖ row-wise and the row-normalised prototypes C ``[K][D]``:

    S_v = ẑ_v·Cᵀ                      E_v = exp(S_v / ε)                     (ε = 0.05, detached)
    r = E_vᵀ·v (v = 1 at first);  u = 1/(K·r);  c = E_v·u;  v = 1/(N·c)      × iters (3)
    q_v[b][k] = u_k·E_v[b][k] / c_b                                          (Σ_k q_v[b][k] = 1)
    p_v = softmax(S_v / τ) row-wise                                          (τ = 0.1)
    L = −1/(2N)·Σ_b Σ_k (q_2·log p_1 + q_1·log p_2)

The official code divides E by its total sum first; that factor cancels in the first u, as does the
shift of exp((S − 1)/ε), which keeps E in (0, 1].

* :func:`swav_reference` — plain torch, any device and dtype: the CPU path, ``--backend torch`` and
  the oracle's twin. It takes C as it is (the criterion normalises it).
* :class:`SwAVLoss` — the criterion (losses/twoview.py); on the GPU it runs the native kernels
  (ops/swav.py).

With W ranks N is the global batch per view: r is summed over the process group in every iteration
(no gradient flows through the codes), c stays local, and the loss is summed differentiably.
"""
from __future__ import annotations

import logging

import torch
import torch.nn.functional as F

from ..ops import swav
from ..parallel import comm
from .twoview import TwoViewLoss


def _codes(S: torch.Tensor, eps: float, iters: int, n: int) -> torch.Tensor:
    E = torch.exp((S - 1) / eps)
    K = S.shape[1]
    r = comm.all_reduce_sum_(E.sum(0))
    for it in range(iters):
        u = 1 / (K * r)
        c = E @ u
        if it + 1 < iters:
            r = comm.all_reduce_sum_((E / (n * c)[:, None]).sum(0))
    return u * E / c[:, None]


def swav_reference(z1: torch.Tensor, z2: torch.Tensor, C: torch.Tensor, eps: float = 0.05, temp: float = 0.1,
                   iters: int = 3) -> torch.Tensor:
    """The loss of the global batch from this rank's rows (differentiable in z1, z2 and C; the same
    value on every rank)."""
    dt = torch.promote_types(torch.promote_types(z1.dtype, z2.dtype), torch.float32)
    n = z1.shape[0] * comm.world_size()
    S = [F.normalize(z.to(dt), dim=1) @ C.to(dt).t() for z in (z1, z2)]
    with torch.no_grad():
        q = [_codes(s, eps, iters, n) for s in S]
    logp = [torch.log_softmax(s / temp, dim=1) for s in S]
    local = -((q[1] * logp[0]).sum() + (q[0] * logp[1]).sum())
    return comm.all_reduce_with_grad(local) / (2 * n)


class SwAVLoss(TwoViewLoss):
    """``prototypes``: the model's prototype weight ``[K][D]``. The criterion keeps a reference (the
    parameter stays registered in the model alone) and normalises its rows in place, without gradient,
    before every forward, as the official ``normalize(w, dim=1); copy_`` does. While
    :meth:`set_frozen` is on, the prototypes' gradient is zero."""
    name, ops = "SwAV", swav

    def __init__(self, prototypes: torch.Tensor, eps: float = 0.05, temp: float = 0.1, iters: int = 3,
                 backend: str = "auto"):
        super().__init__(backend)
        if prototypes.dim() != 2 or prototypes.shape[0] < 2:
            raise ValueError("prototypes must be [K][D] with K >= 2")
        if not (eps > 0 and temp > 0 and iters >= 1):
            raise ValueError("eps > 0, temp > 0 and iters >= 1 are required")
        self._proto = (prototypes,)     # in a tuple: not registered a second time
        self.eps, self.temp, self.iters = float(eps), float(temp), int(iters)
        self.frozen = False

    @property
    def prototypes(self) -> torch.Tensor:
        return self._proto[0]

    def set_frozen(self, frozen: bool) -> None:
        self.frozen = bool(frozen)

    def _use_native(self, z1, n_total):
        C = self.prototypes
        if not super()._use_native(z1, n_total):
            return False
        if self.backend == "auto" and not (C.is_cuda and C.dtype == torch.float32 and C.is_contiguous()
                                          and swav.supported(z1.shape[0], z1.shape[1], C.shape[0], self.iters)):
            if not self._warned:
                self._warned = True
                logging.warning(f"SwAV: prototypes {tuple(C.shape)} ({C.dtype}, {C.device.type}) are outside the "
                                f"native kernels' range (contiguous fp32 GPU, K in [{swav.MIN_K}, {swav.MAX_K}]); "
                                f"using the torch loss")
            return False
        return True

    def native(self, z1, z2):
        # swav_prep normalises the prototypes in place
        return swav.swav_loss(z1, z2, self.prototypes, self.eps, self.temp, self.iters, self.frozen)

    def twin(self, z1, z2):
        C = self.prototypes
        with torch.no_grad():
            C.copy_(F.normalize(C, dim=1))
        return swav_reference(z1, z2, C.detach() if self.frozen else C, self.eps, self.temp, self.iters)
