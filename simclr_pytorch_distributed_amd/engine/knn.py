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

ImageFolder runs (``resize > 0``): either store may be ragged (flat bytes + ``offs``/``hw``), and
every image goes through Resize(resize) + CenterCrop(size) on the GPU (AugConfig.center_crop), so
the bank is the training store as it is resident for pretraining; no cropped copy is made.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from ..data.augment import AugConfig, augment, nhwc8_to_nchw
from ..ops import knn as knn_ops
from ..parallel import comm


class KnnEvaluator:
    def __init__(self, model: torch.nn.Module, backend: str, precision: str, bank_x: torch.Tensor,
                 bank_y: torch.Tensor, val_x: torch.Tensor, val_y: torch.Tensor, mean, std, size: int, n_cls: int,
                 k: int = 200, T: float = 0.1, batch_size: int = 512, runner=None, *, bank_offs=None, bank_hw=None,
                 val_offs=None, val_hw=None, resize: int = 0):
        self.model = model
        self.backend = backend
        self.precision = precision
        self.bank_x, self.bank_y = bank_x, bank_y.long()
        self.val_x, self.val_y = val_x, val_y.long()
        if (bank_offs is None) != (bank_hw is None) or (val_offs is None) != (val_hw is None):
            raise ValueError("offs and hw of a ragged store must be given together")
        if resize <= 0 and (bank_offs is not None or val_offs is not None):
            raise ValueError("a ragged store needs resize > 0 (Resize + CenterCrop)")
        # store tensor -> its (offs, hw), (None, None) for a dense one
        self._ragged = {id(self.bank_x): (bank_offs, bank_hw), id(self.val_x): (val_offs, val_hw)}
        self.aug = (AugConfig.center_crop(size, mean, std, resize) if resize > 0
                    else AugConfig.evaluation(size, mean, std))
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
    @torch.no_grad()
    def _count(self, images: torch.Tensor) -> int:
        """Images in a store: by index, not by the (flat, when ragged) tensor's first dimension."""
        offs = self._ragged.get(id(images), (None, None))[0]
        return int(offs.shape[0]) if offs is not None else int(images.shape[0])

    def _encode_range(self, images: torch.Tensor, lo: int, hi: int, encode) -> torch.Tensor:
        """Features of images lo..hi-1 (indices >= the image count repeat the last image)."""
        n = self._count(images)
        offs, hw = self._ragged.get(id(images), (None, None))
        dev = images.device
        outs = []
        for s in range(lo, hi, self.batch_size):
            idx = torch.arange(s, min(s + self.batch_size, hi), device=dev).clamp_(max=n - 1)
            x = augment(images, idx, self.aug, 0, offs, hw)
            outs.append(F.normalize(encode(x).float(), dim=1))
        return torch.cat(outs) if outs else torch.zeros((0, 0), device=dev)

    def _encoder_fn(self):
        """The eval-mode encoder forward and a function that undoes what it had to set."""
        if self.backend == "native":
            from ..ops.linear_probe import FoldedEncoder
            # rebuilt at every evaluation: the encoder trains between evaluations
            folded = FoldedEncoder(self.model.encoder)
            return folded, (lambda: None)
        enc = self.model.encoder
        flags = [(m, m.training) for m in enc.modules()]
        enc.eval()

        def restore():
            for m, t in flags:
                m.training = t

        return (lambda x: self.runner.encode(nhwc8_to_nchw(x), training=False)), restore

    @torch.no_grad()
    def extract(self, images: torch.Tensor, lo: int = 0, hi: Optional[int] = None) -> torch.Tensor:
        """L2-normalised fp32 encoder features (not the projection head's) of ``images[lo:hi]``."""
        encode, restore = self._encoder_fn()
        try:
            return self._encode_range(images, lo, self._count(images) if hi is None else hi, encode)
        finally:
            restore()

    @torch.no_grad()
    def evaluate(self) -> Tuple[float, float]:
        """(top-1, top-5) of the validation set in percent; identical on every rank."""
        W, r = comm.world_size(), comm.rank()
        nb, nv = self._count(self.bank_x), self._count(self.val_x)
        per_b, per_v = (nb + W - 1) // W, (nv + W - 1) // W
        encode, restore = self._encoder_fn()
        try:
            bank_f = self._encode_range(self.bank_x, r * per_b, (r + 1) * per_b, encode)
            v_lo, v_hi = min(r * per_v, nv), min((r + 1) * per_v, nv)
            q = self._encode_range(self.val_x, v_lo, v_hi, encode)
        finally:
            restore()
        if W > 1:
            bank_f = comm.all_gather_tensor(bank_f)[:nb]     # slices are contiguous: pad rows sit at the end
        self.last_bank = bank_f
        hits = torch.zeros(2, dtype=torch.float32, device=bank_f.device)
        if v_hi > v_lo:
            native = self.backend == "native"
            _, st = knn_ops.knn_classify(q, bank_f, self.bank_y, self.n_cls, self.k, self.T,
                                         labels=self.val_y[v_lo:v_hi],
                                         backend="auto" if native else "torch")
            hits = st.to(torch.float32)
        if W > 1:
            hits = hits.clone()
            comm.all_reduce_sum_(hits)
        h1, h5 = hits.tolist()
        return 100.0 * h1 / nv, 100.0 * h5 / nv
