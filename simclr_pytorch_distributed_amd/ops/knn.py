"""Weighted k-NN classification of L2-normalised features (the InstDisc / MoCo / SimCLR
monitor protocol): each query takes its ``k`` nearest bank rows by cosine similarity and
class ``c`` receives the vote Σ exp(sim / T) over the neighbours of class ``c``.

* :func:`knn_reference` — pure torch, any device and dtype: the CPU path and the oracle.
* :func:`knn_classify` — the native gfx950 kernels (csrc/kernels/knn.hip: MFMA similarity
  tiles with a running per-query top-k, the Nq x Nb matrix never materialised, then the
  vote kernel) when the tensors are on the GPU and the shape is supported, else the
  reference. A native request that cannot be served raises; it never falls back silently.

Neighbour order everywhere: similarity descending, then bank index ascending.
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import torch

from . import _ext

MAX_K = 256          # list capacity of the native kernel
MAX_CLASSES = 1024


def supported(D: int, n_cls: int, k: int) -> bool:
    """Shapes the native kernels take: D = 64·2^j <= 2048, n_cls <= 1024, 1 <= k <= 256."""
    j = D // 64
    return D % 64 == 0 and 64 <= D <= 2048 and (j & (j - 1)) == 0 and 1 <= n_cls <= MAX_CLASSES and 1 <= k <= MAX_K


def _canonical(v: torch.Tensor, i: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Order each row's (value, index) pairs by value descending, then index ascending."""
    i, perm = torch.sort(i, dim=1)
    v = v.gather(1, perm)
    v, perm = torch.sort(v, dim=1, descending=True, stable=True)
    return v.contiguous(), i.gather(1, perm).contiguous()


def _topk_sorted(sim: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k largest entries per row by (similarity descending, index ascending).

    ``torch.topk`` leaves open which of several entries equal to the k-th value it returns,
    so rows with such a tie at the boundary go through a stable descending sort of the whole
    row (equal similarities keep their ascending index order); the others only have their k
    entries put into the canonical order."""
    v, i = torch.topk(sim, k, dim=1)
    v, i = _canonical(v, i)
    tied = ((sim >= v[:, -1:]).sum(dim=1) > k).nonzero().flatten()
    if tied.numel():
        fv, fi = torch.sort(sim[tied], dim=1, descending=True, stable=True)
        v[tied], i[tied] = fv[:, :k], fi[:, :k]
    return v, i


def knn_reference(q: torch.Tensor, bank: torch.Tensor, bank_labels: torch.Tensor, n_cls: int, k: int, T: float,
                  chunk: int = 1024):
    """``(scores [Nq][n_cls], sims [Nq][k], idx [Nq][k])`` in the dtype and on the device of
    ``q``; queries go through the similarity matmul in chunks of ``chunk`` rows."""
    nb = bank.shape[0]
    k = int(min(k, nb))
    bank = bank.to(q.dtype)
    labels = bank_labels.long()
    sims, idxs, scores = [], [], []
    for s in range(0, q.shape[0], chunk):
        v, i = _topk_sorted(q[s:s + chunk] @ bank.t(), k)
        w = torch.exp(v / T)
        lab = labels[i]
        sc = torch.zeros(v.shape[0], n_cls, dtype=q.dtype, device=q.device)
        # one neighbour rank at a time: a row adds to one class per call, so the sum runs in
        # list order on every device (a whole-list scatter_add is unordered atomics on a GPU)
        for j in range(k):
            sc.scatter_add_(1, lab[:, j:j + 1], w[:, j:j + 1])
        sims.append(v)
        idxs.append(i)
        scores.append(sc)
    if not sims:
        z = q.new_zeros((0, k))
        return q.new_zeros((0, n_cls)), z, z.long()
    return torch.cat(scores), torch.cat(sims), torch.cat(idxs)


def hit_counts(scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``[hits@1, hits@5]`` with the rank rule of the linear-probe kernel: the label's rank is
    #{c : score_c > score_label}; a hit@kk is rank < kk."""
    own = scores.gather(1, labels.long()[:, None])
    rank = (scores > own).sum(dim=1)
    return torch.stack([(rank < 1).sum(), (rank < 5).sum()]).to(torch.float32)


def knn_topk(q: torch.Tensor, bank: torch.Tensor, k: int, n_split: int = 0):
    """Native top-k: ``(sims [Nq][k] fp32, idx [Nq][k] int32)``."""
    out = _ext.require().knn_topk(q, bank, int(k), int(n_split))
    return out[0], out[1]


def knn_vote(sims: torch.Tensor, idx: torch.Tensor, bank_labels: torch.Tensor, n_cls: int, T: float,
             labels: Optional[torch.Tensor] = None):
    """Native vote: ``(scores [Nq][n_cls], stats [2] = hits@1, hits@5 when labels are given)``."""
    out = _ext.require().knn_vote(sims, idx, bank_labels, int(n_cls), float(T), labels)
    return out[0], out[1]


def knn_classify(q: torch.Tensor, bank: torch.Tensor, bank_labels: torch.Tensor, n_cls: int, k: int = 200,
                 T: float = 0.1, labels: Optional[torch.Tensor] = None, backend: str = "auto"):
    """Weighted k-NN scores of ``q`` against ``bank``. Returns ``(scores, stats)``; ``stats`` is
    ``[hits@1, hits@5]`` (fp32) when ``labels`` is given, else None.

    ``backend``: ``native`` (raises when the kernels cannot take the call), ``torch`` (the
    reference) or ``auto`` (native when the tensors are on the GPU, the extension is built
    and :func:`supported` holds)."""
    if backend not in ("auto", "native", "torch"):
        raise ValueError(f"backend {backend!r}")
    nb, D = bank.shape[0], q.shape[1]
    if k > nb:
        logging.warning(f"k-NN: k {k} clamped to the bank size {nb}")
        k = nb
    use_native = False
    if backend == "native":
        if not q.is_cuda:
            raise RuntimeError("k-NN native backend needs GPU tensors")
        _ext.require()
        if k > MAX_K:
            logging.warning(f"k-NN: k {k} clamped to the native kernel's capacity {MAX_K}")
            k = MAX_K
        if not supported(D, n_cls, k):
            raise RuntimeError(f"k-NN native backend: unsupported shape D={D}, n_cls={n_cls}, k={k} "
                               "(D = 64·2^j <= 2048, n_cls <= 1024, k <= 256)")
        use_native = True
    elif backend == "auto" and q.is_cuda and _ext.available():
        kk = min(k, MAX_K)
        if supported(D, n_cls, kk):
            if kk < k:
                logging.warning(f"k-NN: k {k} clamped to the native kernel's capacity {MAX_K}")
            k = kk
            use_native = True
    if use_native:
        sims, idx = knn_topk(q.float().contiguous(), bank.float().contiguous(), k)
        scores, stats = knn_vote(sims, idx, bank_labels.long().contiguous(), n_cls, T,
                                 labels.long().contiguous() if labels is not None else None)
        return scores, (stats if labels is not None else None)
    scores, _, _ = knn_reference(q, bank, bank_labels, n_cls, k, T)
    return scores, (hit_counts(scores, labels) if labels is not None else None)
