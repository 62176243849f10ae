"""Weighted k-NN evaluation of the encoder (ops/knn.py): a label-based quality number that
needs no training — the training set's L2-normalised encoder features form the bank, every
validation image votes with its ``k`` nearest bank rows, top-1 / top-5 are reported.

The evaluator reads the model and changes nothing a training run depends on: parameters,
BatchNorm statistics and counters, ``module.training`` flags, the flat buffers, the weight
cache, the step seed and the torch RNG state are the same after :meth:`KnnEvaluator.evaluate`
as before it.

Several ranks: every rank encodes a contiguous 1/W slice of the bank and of the queries (the
last slices padded to equal length by repeating the final image; pad rows are dropped by
index after the gather), the bank features are all-gathered, the hit counts summed.

ImageFolder runs (``aug.resize > 0``): either store may be ragged (data/store.py), and
every image goes through Resize(resize) + CenterCrop(size) on the GPU (AugConfig.center_crop), so
the bank is the training store as it is resident for pretraining; no cropped copy is made.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ..data.augment import AugConfig
from ..data.store import DeviceStore
from ..ops import knn as knn_ops
from ..ops.linear_probe import eval_encoder
from ..parallel import comm


class KnnEvaluator:
    def __init__(self, model: torch.nn.Module, backend: str, precision: str, bank: DeviceStore, val: DeviceStore,
                 aug: AugConfig, n_cls: int, k: int = 200, T: float = 0.1, batch_size: int = 512, runner=None):
        self.model = model
        self.backend = backend
        self.precision = precision
        self.bank, self.val = bank, val
        self._bank_y, self._val_y = bank.labels.long(), val.labels.long()
        if aug.resize <= 0 and (bank.ragged or val.ragged):
            raise ValueError("a ragged store needs resize > 0 (Resize + CenterCrop)")
        self.aug = aug          # AugConfig.evaluation, or .center_crop of an ImageFolder run
        self.n_cls = int(n_cls)
        self.k = int(k)
        self.T = float(T)
        self.batch_size = int(batch_size)
        if runner is None and backend != "native":
            from ..models.executor import ModelRunner
            runner = ModelRunner(model, backend, precision)
        self.runner = runner
        self.last_bank: Optional[torch.Tensor] = None   # gathered bank features of the last evaluate()

    # --------------------------------------------------------------------------------
    def _encode_range(self, store: DeviceStore, lo: int, hi: int, encode) -> torch.Tensor:
        """Features of images lo..hi-1 (indices >= the image count repeat the last image)."""
        n = len(store)
        dev = store.images.device
        outs = []
        for s in range(lo, hi, self.batch_size):
            idx = torch.arange(s, min(s + self.batch_size, hi), device=dev).clamp_(max=n - 1)
            outs.append(F.normalize(encode(store.views(idx, self.aug, 0)), dim=1))
        return torch.cat(outs) if outs else torch.zeros((0, 0), device=dev)

    @torch.no_grad()
    def extract(self, store: DeviceStore, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
        """L2-normalised fp32 encoder features (not the projection head's) of images lo..hi-1 of ``store``."""
        # the fold of NOW: the encoder trains between evaluations
        encode, restore = eval_encoder(self.model, self.backend, self.runner)
        try:
            return self._encode_range(store, lo, len(store) if hi is None else hi, encode)
        finally:
            restore()

    @torch.no_grad()
    def evaluate(self) -> Tuple[float, float]:
        """(top-1, top-5) of the validation set in percent; identical on every rank."""
        W, r = comm.world_size(), comm.rank()
        nb, nv = len(self.bank), len(self.val)
        per_b, per_v = (nb + W - 1) // W, (nv + W - 1) // W
        # the fold of NOW: the encoder trains between evaluations
        encode, restore = eval_encoder(self.model, self.backend, self.runner)
        try:
            bank_f = self._encode_range(self.bank, r * per_b, (r + 1) * per_b, encode)
            v_lo, v_hi = min(r * per_v, nv), min((r + 1) * per_v, nv)
            q = self._encode_range(self.val, v_lo, v_hi, encode)
        finally:
            restore()
        if W > 1:
            bank_f = comm.all_gather_tensor(bank_f)[:nb]     # slices are contiguous: pad rows sit at the end
        self.last_bank = bank_f
        hits = torch.zeros(2, dtype=torch.float32, device=bank_f.device)
        if v_hi > v_lo:
            native = self.backend == "native"
            _, st = knn_ops.knn_classify(q, bank_f, self._bank_y, self.n_cls, self.k, self.T,
                                         labels=self._val_y[v_lo:v_hi],
                                         backend="auto" if native else "torch")
            hits = st.to(torch.float32)
        if W > 1:
            hits = hits.clone()
            comm.all_reduce_sum_(hits)
        h1, h5 = hits.tolist()
        return 100.0 * h1 / nv, 100.0 * h5 / nv
