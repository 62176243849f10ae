"""Native linear evaluation (reference main_linear.py:119-244,
networks/resnet_big.py:196-204).

* :class:`FoldedEncoder` — the frozen encoder in eval mode with every BatchNorm folded into
  its conv: W' = W·γ/√(σ²+ε) per output channel, b' = β − μ·γ/√(σ²+ε). Each conv (+BN +ReLU)
  is ONE implicit-GEMM launch whose epilogue adds b' (and applies the ReLU) on the fp32
  accumulators before the bf16 rounding; a block output is relu(y3' + shortcut) in one
  elementwise pass. No BatchNorm kernel runs at all. The encoder is frozen for the whole
  probe, so the fold is computed once.
* :class:`NativeLinearCE` — ``LinearClassifier`` + ``CrossEntropyLoss`` + top-1/5 +
  ``torch.optim.SGD`` as two fused launches per batch (csrc/kernels/linear_ce.hip), fp32 as
  the reference classifier; the statistics stay on the device.
* :class:`NativeLinearSweep` — G such classifiers, each with its own learning rate and weight
  decay, on one feature batch in the same two launches (csrc/kernels/linear_ce_sweep.hip): a
  hyper-parameter sweep of the probe pays for the encoder once.
* :class:`FeatureBank` — the frozen encoder's features of a whole store, extracted once
  (``--cache_features``); ``train_batch_rows`` / ``eval_batch_rows`` of the two classes above
  read a batch from it by row index inside the same launches (no gather, no copy).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import _ext
from .pool import global_avgpool_nhwc, maxpool_nhwc
from ..models.resnet import Bottleneck


def _fold(conv: torch.nn.Conv2d, bn: torch.nn.BatchNorm2d, c_pad: int = 0):
    """bf16 KRSC weights and fp32 bias of conv followed by eval-mode bn."""
    w = conv.weight.detach().float()
    inv = torch.rsqrt(bn.running_var.float() + bn.eps)
    g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(inv)
    b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(inv)
    scale = g * inv
    wk = (w * scale[:, None, None, None]).permute(0, 2, 3, 1)            # [K][R][S][C]
    if c_pad > wk.shape[-1]:
        wk = torch.nn.functional.pad(wk, (0, c_pad - wk.shape[-1]))
    bias = (b - bn.running_mean.float() * scale).contiguous()
    return wk.to(torch.bfloat16).contiguous(), bias


class FoldedEncoder:
    """Eval-mode native forward of a ``models.resnet.ResNet`` with folded BatchNorm."""

    def __init__(self, enc, c_pad: int = 8):
        self.enc = enc
        self.stem = getattr(enc, "stem", "cifar")
        self.w0, self.b0 = _fold(enc.conv1, enc.bn1, c_pad)
        self.blocks: List[Dict] = []
        for blk in enc.blocks():
            d: Dict = {"bottle": isinstance(blk, Bottleneck), "stride": blk.stride}
            d["c1"] = _fold(blk.conv1, blk.bn1)
            d["c2"] = _fold(blk.conv2, blk.bn2)
            if d["bottle"]:
                d["c3"] = _fold(blk.conv3, blk.bn3)
            d["sc"] = _fold(blk.shortcut[0], blk.shortcut[1]) if len(blk.shortcut) > 0 else None
            self.blocks.append(d)
        dev = self.b0.device
        self._ones, self._zeros = {}, {}
        for d in self.blocks:
            c = (d["c3"] if d["bottle"] else d["c2"])[1].numel()
            self._ones.setdefault(c, torch.ones(c, device=dev))
            self._zeros.setdefault(c, torch.zeros(c, device=dev))

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """``x``: NHWC bf16 [N, H, W, 8] -> fp32 features [N, feat_dim]."""
        m = _ext.require()
        if self.stem == "cifar":
            out = m.conv_fwd_bias(x, self.w0, 1, 1, self.b0, True)
        else:
            out = maxpool_nhwc(m.conv_fwd_bias(x, self.w0, 2, 3, self.b0, True), 3, 2, 1)
        for d in self.blocks:
            st = d["stride"]
            if d["bottle"]:
                a1 = m.conv_fwd_bias(out, d["c1"][0], 1, 0, d["c1"][1], True)
                a2 = m.conv_fwd_bias(a1, d["c2"][0], st, 1, d["c2"][1], True)
                y = m.conv_fwd_bias(a2, d["c3"][0], 1, 0, d["c3"][1], False)
            else:
                a1 = m.conv_fwd_bias(out, d["c1"][0], st, 1, d["c1"][1], True)
                y = m.conv_fwd_bias(a1, d["c2"][0], 1, 1, d["c2"][1], False)
            sc = m.conv_fwd_bias(out, d["sc"][0], st, 0, d["sc"][1], False) if d["sc"] is not None else out
            c = y.shape[-1]
            out = m.bn_apply(y, self._ones[c], self._zeros[c], sc, None, None, 2, True, None)   # relu(y + sc)
        return global_avgpool_nhwc(out)


def eval_encoder(model: torch.nn.Module, backend: str, runner=None):
    """(encode, restore): ``encode`` maps an NHWC batch (data/augment.py) to the fp32 features of
    ``model.encoder`` in eval mode, ``restore`` undoes what that had to set. native: a
    :class:`FoldedEncoder` of the weights and statistics of NOW (a caller whose encoder trains
    asks again at every evaluation), nothing to restore; torch: ``runner.encode`` after the
    encoder's ``training`` flags were recorded and ``eval()`` set."""
    if backend == "native":
        return FoldedEncoder(model.encoder), (lambda: None)
    from ..data.augment import nhwc8_to_nchw
    enc = model.encoder
    flags = [(m, m.training) for m in enc.modules()]
    enc.eval()

    def restore():
        for m, t in flags:
            m.training = t

    @torch.no_grad()
    def encode(x):
        return runner.encode(nhwc8_to_nchw(x), training=False).float()

    return encode, restore


class NativeLinearCE:
    """``LinearClassifier`` trained with cross-entropy and SGD on the native path. Holds its
    own momentum buffers (the linear probe writes no checkpoint, main_linear.py)."""

    def __init__(self, classifier: torch.nn.Module, momentum: float = 0.9, weight_decay: float = 0.0,
                 gemm: str = "fma"):
        fc = classifier.fc
        self.gemm = _check_gemm(gemm)
        self.W, self.b = fc.weight, fc.bias
        self.momentum = float(momentum)
        self.weight_decay = float(weight_decay)
        self.bufW = torch.zeros_like(self.W)
        self.bufb = torch.zeros_like(self.b)
        self.first = True

    def train_batch(self, feats: torch.Tensor, labels: torch.Tensor, lr: float):
        """One SGD step on the batch; returns (logits, stats [Σ CE, hits@1, hits@5]) on device."""
        with torch.no_grad():
            out = self._op()(feats.float().contiguous(), self.W.data, self.b.data, labels.long(),
                             self.bufW, self.bufb, float(lr), self.momentum, self.weight_decay, self.first, True)
        self.first = False
        return out[0], out[1]

    @torch.no_grad()
    def eval_batch(self, feats: torch.Tensor, labels: torch.Tensor):
        out = self._op()(feats.float().contiguous(), self.W.data, self.b.data, labels.long(),
                         None, None, 0.0, 0.0, 0.0, False, False)
        return out[0], out[1]

    @torch.no_grad()
    def train_batch_rows(self, bank: torch.Tensor, bank_labels: torch.Tensor, rows: torch.Tensor, lr: float):
        """``train_batch(bank[rows], bank_labels[rows], lr)``, bit for bit, with the rows read from
        the bank in place: ``bank`` fp32 [N, K], ``bank_labels`` int64 [N], ``rows`` int64 [B] on
        the device, every value in [0, N)."""
        out = self._op(True)(bank, self.W.data, self.b.data, bank_labels, rows, self.bufW, self.bufb,
                             float(lr), self.momentum, self.weight_decay, self.first, True)
        self.first = False
        return out[0], out[1]

    @torch.no_grad()
    def eval_batch_rows(self, bank: torch.Tensor, bank_labels: torch.Tensor, rows: torch.Tensor):
        out = self._op(True)(bank, self.W.data, self.b.data, bank_labels, rows, None, None, 0.0, 0.0, 0.0,
                             False, False)
        return out[0], out[1]

    def _op(self, rows: bool = False):
        m = _ext.require()
        if rows:
            return m.linear_ce_step_mfma_rows if self.gemm == "mfma" else m.linear_ce_step_rows
        return m.linear_ce_step_mfma if self.gemm == "mfma" else m.linear_ce_step


SWEEP_MAX_HEADS = 16


class NativeLinearSweep:
    """G copies of a ``LinearClassifier`` trained side by side on the same features, head g
    with its own learning rate and weight decay: two launches per batch for all of them
    (csrc/kernels/linear_ce_sweep.hip). Every head starts from ``classifier``'s weights and is
    bit-identical to a :class:`NativeLinearCE` run alone with its settings."""

    def __init__(self, classifier: torch.nn.Module, weight_decays: Sequence[float], momentum: float = 0.9,
                 gemm: str = "fma"):
        fc = classifier.fc
        self.gemm = _check_gemm(gemm)
        self.G = len(weight_decays)
        if not 1 <= self.G <= SWEEP_MAX_HEADS:
            raise ValueError(f"a sweep has 1..{SWEEP_MAX_HEADS} heads, got {self.G}")
        self.W = fc.weight.detach().unsqueeze(0).repeat(self.G, 1, 1).contiguous()
        self.b = fc.bias.detach().unsqueeze(0).repeat(self.G, 1).contiguous()
        self.momentum = float(momentum)
        self.weight_decays = [float(w) for w in weight_decays]
        self.bufW = torch.zeros_like(self.W)
        self.bufb = torch.zeros_like(self.b)
        self.first = True

    @torch.no_grad()
    def train_batch(self, feats: torch.Tensor, labels: torch.Tensor, lrs: Sequence[float]):
        """One SGD step of every head; returns (logits [G, B, C], stats [G, 3]) on device."""
        out = self._op()(feats.float().contiguous(), self.W, self.b, labels.long(),
                         self.bufW, self.bufb, [float(v) for v in lrs], self.momentum,
                         self.weight_decays, self.first, True)
        self.first = False
        return out[0], out[1]

    @torch.no_grad()
    def eval_batch(self, feats: torch.Tensor, labels: torch.Tensor):
        zeros = [0.0] * self.G
        out = self._op()(feats.float().contiguous(), self.W, self.b, labels.long(),
                         None, None, zeros, 0.0, zeros, False, False)
        return out[0], out[1]

    @torch.no_grad()
    def train_batch_rows(self, bank: torch.Tensor, bank_labels: torch.Tensor, rows: torch.Tensor,
                         lrs: Sequence[float]):
        """``train_batch(bank[rows], bank_labels[rows], lrs)``, bit for bit, the rows read in place
        (see :meth:`NativeLinearCE.train_batch_rows`)."""
        out = self._op(True)(bank, self.W, self.b, bank_labels, rows, self.bufW, self.bufb,
                             [float(v) for v in lrs], self.momentum, self.weight_decays, self.first, True)
        self.first = False
        return out[0], out[1]

    @torch.no_grad()
    def eval_batch_rows(self, bank: torch.Tensor, bank_labels: torch.Tensor, rows: torch.Tensor):
        zeros = [0.0] * self.G
        out = self._op(True)(bank, self.W, self.b, bank_labels, rows, None, None, zeros, 0.0, zeros, False, False)
        return out[0], out[1]

    def _op(self, rows: bool = False):
        m = _ext.require()
        if rows:
            return m.linear_ce_sweep_step_mfma_rows if self.gemm == "mfma" else m.linear_ce_sweep_step_rows
        return m.linear_ce_sweep_step_mfma if self.gemm == "mfma" else m.linear_ce_sweep_step

    def head_state(self, g: int) -> Dict[str, torch.Tensor]:
        """``LinearClassifier`` state dict of head ``g``."""
        return {"fc.weight": self.W[g].clone(), "fc.bias": self.b[g].clone()}


class FeatureBank:
    """Features of a store under the frozen encoder, extracted once: ``feats`` fp32 [V·N, K] with
    row ``v·N + i`` = view ``v`` of image ``i`` (one view: the evaluation transform), ``labels``
    int64 [V·N] repeated alike, so a row index addresses both."""

    def __init__(self, feats: torch.Tensor, labels: torch.Tensor, n_images: int, views: int = 1):
        if feats.shape[0] != n_images * views or labels.shape[0] != feats.shape[0]:
            raise ValueError("a bank holds views x images rows of features and as many labels")
        self.feats, self.labels, self.n, self.views = feats, labels, int(n_images), int(views)

    def rows_for(self, idx: torch.Tensor, epoch: int) -> torch.Tensor:
        """Bank rows of images ``idx`` in ``epoch`` (1-based): every image uses view (epoch − 1) mod V."""
        v = (epoch - 1) % self.views
        return idx if v == 0 else idx + v * self.n

    def epoch_view(self, epoch: int):
        """(feats [N, K], labels [N]) of ``epoch``'s view: slices of the bank, so the sampler's own
        image indices are its rows and a training step launches nothing to translate them."""
        v = (epoch - 1) % self.views
        return self.feats[v * self.n:(v + 1) * self.n], self.labels[v * self.n:(v + 1) * self.n]

    @staticmethod
    def nbytes(rows: int, feat_dim: int) -> int:
        """Bytes of a bank of ``rows`` rows: fp32 features + int64 labels."""
        return rows * (feat_dim * 4 + 8)


GEMMS = ("fma", "mfma")


def _check_gemm(gemm: str) -> str:
    if gemm not in GEMMS:
        raise ValueError(f"gemm must be one of {GEMMS}, got {gemm!r}")
    return gemm


def shape_supported(k: int, c: int, gemm: str = "fma") -> bool:
    """The (feature, class) range of the classifier kernels: ``fma`` K = 64·2^j <= 2048 and
    C <= 1024 (linear_ce.hip), ``mfma`` K = 64·j <= 4096 and C <= 32768 (head_gemm.hip)."""
    if _check_gemm(gemm) == "mfma":
        return k % 64 == 0 and 64 <= k <= 4096 and 1 <= c <= 32768
    return k % 64 == 0 and k <= 2048 and ((k // 64) & (k // 64 - 1)) == 0 and c <= 1024


def supported(classifier: torch.nn.Module, feat_dim: Optional[int] = None, gemm: str = "fma") -> bool:
    fc = getattr(classifier, "fc", None)
    _check_gemm(gemm)
    if fc is None or not fc.weight.is_cuda or not _ext.available():
        return False
    return shape_supported(fc.in_features, fc.out_features, gemm)


def sweep_supported(classifier: torch.nn.Module, G: int, gemm: str = "fma") -> bool:
    if not (1 <= G <= SWEEP_MAX_HEADS and supported(classifier, gemm=gemm)):
        return False
    fc = classifier.fc
    return gemm == "fma" or G * fc.out_features * fc.in_features < 2 ** 31
