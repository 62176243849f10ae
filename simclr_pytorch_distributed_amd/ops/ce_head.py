"""Trainable classifier + cross-entropy (reference main_ce.py / networks/resnet_big.py:184-193:
``SupCEResNet.fc`` on the encoder features, ``nn.CrossEntropyLoss`` (mean), ``util.accuracy``
top-1 / top-5) as ONE autograd node of two launches per step (csrc/kernels/linear_ce.hip).

* forward: ``linear_ce_fwd`` — logits, per-row loss and top-1/5 hits, and
  dz = (softmax − onehot) / B, the gradient of the mean loss with respect to the logits;
* backward: ``ce_head_bwd`` — dX = gout·dz·W returned to autograd, dW += gout·dzᵀ·x and
  db += gout·Σ_b dz accumulated straight into the parameter sinks (``ops/sinks.py``: the views
  of the flat gradient buffer), and the row statistics summed in row order.

fp32 throughout and deterministic (no atomics, fixed summation order).

The statistics are summed by the backward launch: ``loss`` and ``stats`` hold their values once
``loss.backward()`` has been queued (stream order), which is where a training step reads them.
A forward that records no graph (``torch.no_grad()``, or nothing requires a gradient) sums them
itself, so its outputs are valid at once.

Unsupported shapes (K ≠ 64·2^j, K > 2048, C > 1024), CPU tensors and the ``torch`` backend use
``F.linear`` + ``F.cross_entropy``: the same values through stock torch ops.

``gemm="mfma"`` (``--head_gemm mfma``) runs the three GEMMs of the node on split-bf16 MFMA
kernels (csrc/kernels/head_gemm.hip) for any K = 64·j <= 4096 and C <= 32768: two launches
forward, two backward, the same outputs, sinks and statistics convention. The default stays
``fma``.

Soft targets (``labels2`` / ``lam`` / ``smoothing``: Mixup, CutMix, label smoothing): the target of
a row with labels a, b is t_c = (1 − ε)·(λ·[c = a] + (1 − λ)·[c = b]) + ε/C. Only the forward's row
softmax changes (``ce_head_fwd_soft[_mfma]``: loss = lse − Σ_c t_c·z_c, dz = (softmax − t) / B, hits
against a); the backward launches read dz and are the same ops. With the defaults the node is the
plain one, launch for launch.

Knowledge distillation (``teacher_logits`` / ``temp`` / ``alpha``): with q_t = softmax(v / τ) of the
teacher's logits v and q_s = softmax(z / τ), loss = (1 − α)·CE(z, t) + α·τ²·KL(q_t ‖ q_s) (batch mean),
t the soft target above. Again only the forward's row softmax changes (``ce_head_fwd_distill[_mfma]``,
csrc/include/distill_ce.h); the backward launches are the same ops, and the teacher's logits never
receive a gradient. α = 1 forms no CE term: a label outside [0, C) is then allowed (an unlabelled
image) and scores no hit. Without ``teacher_logits`` the call is today's, launch for launch.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

from . import _ext, sinks


def supported(fc: torch.nn.Linear, gemm: str = "fma") -> bool:
    """Whether the native node can run this classifier (its launchers refuse anything else).
    ``gemm="mfma"``: the range of csrc/kernels/head_gemm.hip (K = 64·j <= 4096, C <= 32768)."""
    from .linear_probe import shape_supported
    ok = shape_supported(fc.in_features, fc.out_features, gemm) and fc.out_features >= 1
    if not fc.weight.is_cuda or fc.bias is None or fc.weight.dtype != torch.float32 or not _ext.available():
        return False
    return ok


class _ClassifierCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, labels, fc, record, gemm, soft, *params):
        m = _ext.require()
        x = feat.detach().float().contiguous()
        w = fc.weight.detach()
        # record: a backward will follow (decided by the caller: grad mode is off in here)
        need = [ctx.needs_input_grad[0], any(ctx.needs_input_grad[6:])]
        if soft is None:
            fwd = m.ce_head_fwd_mfma if gemm == "mfma" else m.ce_head_fwd
            logits, dz, rowstat, stats, loss = fwd(x, w, fc.bias.detach(), labels, not record)
        elif len(soft) == 3:
            labels2, lam, eps = soft
            fwd = m.ce_head_fwd_soft_mfma if gemm == "mfma" else m.ce_head_fwd_soft
            logits, dz, rowstat, stats, loss = fwd(x, w, fc.bias.detach(), labels, labels2, lam, eps, not record)
        else:
            labels2, lam, eps, teacher, temp, alpha = soft
            fwd = m.ce_head_fwd_distill_mfma if gemm == "mfma" else m.ce_head_fwd_distill
            logits, dz, rowstat, stats, loss = fwd(x, w, fc.bias.detach(), labels, labels2, lam, eps, teacher, temp,
                                                   alpha, not record)
        ctx.save_for_backward(x, dz, w, rowstat, stats, loss)
        ctx.fc = fc
        ctx.gemm = gemm
        ctx.params = params
        ctx.need = need
        ctx.feat_dtype = feat.dtype
        ctx.mark_non_differentiable(stats, logits)
        return loss, stats, logits

    @staticmethod
    def backward(ctx, gout, _gstats, _glogits):
        x, dz, w, rowstat, stats, loss = ctx.saved_tensors
        fc = ctx.fc
        need_dx, need_dw = ctx.need
        t = sinks.target
        go = gout.detach().float().contiguous()
        m = _ext.require()
        bwd = m.ce_head_bwd_mfma if ctx.gemm == "mfma" else m.ce_head_bwd
        dx = bwd(x, dz, w, go, rowstat, stats, loss,
                 t(fc.weight) if need_dw else None, t(fc.bias) if need_dw else None, need_dx)
        if need_dw:
            sinks.notify(ctx.params)
        return (dx.to(ctx.feat_dtype) if dx is not None else None,) + (None,) * (5 + len(ctx.params))


def soft_target(labels: torch.Tensor, labels2: torch.Tensor, lam: float, smoothing: float, n_cls: int,
                dtype=torch.float32) -> torch.Tensor:
    """The probability target [B, C]: t_c = (1 − ε)·(λ·[c = a] + (1 − λ)·[c = b]) + ε/C."""
    a = F.one_hot(labels.long(), n_cls).to(dtype)
    b = F.one_hot(labels2.long(), n_cls).to(dtype)
    return (1.0 - smoothing) * (lam * a + (1.0 - lam) * b) + smoothing / n_cls


def distill_loss(logits: torch.Tensor, ce, teacher_logits: torch.Tensor, temp: float, alpha: float) -> torch.Tensor:
    """(1 − α)·ce + α·τ²·KL(softmax(v / τ) ‖ softmax(z / τ)), batch mean, from stock ops; ``ce`` (the mean
    cross-entropy term) is not used at α = 1 and may be None then."""
    kd = F.kl_div(F.log_softmax(logits / temp, 1), F.softmax(teacher_logits.detach().to(logits.dtype) / temp, 1),
                  reduction="batchmean") * (temp * temp)
    return kd if alpha == 1.0 else (1.0 - alpha) * ce + alpha * kd


def classifier_ce_logits(feat: torch.Tensor, fc: torch.nn.Linear, labels: torch.Tensor,
                         native: bool = True, gemm: str = "fma", labels2=None, lam: float = 1.0,
                         smoothing: float = 0.0, teacher_logits=None, temp: float = 1.0,
                         alpha: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss, stats, logits) of ``F.cross_entropy(fc(feat), labels)``: ``loss`` the batch mean,
    ``stats`` = [Σ_rows CE, top-1 hits, top-5 hits] (fp32, no gradient), ``logits`` [B, C] (no
    gradient). ``native=False`` forces the torch ops. ``gemm="mfma"``: the GEMMs of the node on
    csrc/kernels/head_gemm.hip; a classifier outside its range is an error here (the engines decide
    beforehand, with one warning, which path a run takes).

    ``labels2`` / ``lam`` / ``smoothing``: the soft target of the module docstring (``labels2``
    None = ``labels``); the loss is then ``F.cross_entropy(logits, t)`` with the probability target
    and the hits are counted against ``labels``. With the defaults this is the plain path.

    ``teacher_logits`` [B, C] / ``temp`` / ``alpha``: knowledge distillation (module docstring); the
    loss is then the blend of that cross-entropy and τ²·KL to the teacher, ``stats[0]`` its row sum.
    ``teacher_logits`` is a constant: no gradient reaches it."""
    labels = labels.long()
    lam, smoothing = float(lam), float(smoothing)
    if not (0.0 <= lam <= 1.0 and 0.0 <= smoothing < 1.0):
        raise ValueError(f"lam {lam} must be in [0, 1] and smoothing {smoothing} in [0, 1)")
    soft = None
    if labels2 is not None or lam != 1.0 or smoothing != 0.0:
        soft = ((labels if labels2 is None else labels2.long()).contiguous(), lam, smoothing)
    if teacher_logits is not None:
        temp, alpha = float(temp), float(alpha)
        if not (0.0 < temp < float("inf") and 0.0 <= alpha <= 1.0):
            raise ValueError(f"temp {temp} must be finite and > 0 and alpha {alpha} in [0, 1]")
        if tuple(teacher_logits.shape) != (labels.numel(), fc.out_features):
            raise ValueError(f"teacher_logits {tuple(teacher_logits.shape)} must be "
                             f"[{labels.numel()}, {fc.out_features}]")
        teacher_logits = teacher_logits.detach()
        if soft is None:
            soft = (labels.contiguous(), 1.0, 0.0)
        soft = soft + (teacher_logits.float().contiguous(), temp, alpha)
    if native and feat.is_cuda and gemm == "mfma" and not supported(fc, "mfma"):
        raise ValueError(f"gemm='mfma' cannot run a {fc.in_features} x {fc.out_features} classifier")
    if native and feat.is_cuda and supported(fc, gemm):
        record = torch.is_grad_enabled() and (feat.requires_grad or fc.weight.requires_grad or fc.bias.requires_grad)
        return _ClassifierCE.apply(feat, labels.contiguous(), fc, record, gemm, soft, fc.weight, fc.bias)
    logits = F.linear(feat.float(), fc.weight, fc.bias)
    valid = None
    if soft is None:
        loss = F.cross_entropy(logits, labels)
    elif len(soft) == 6 and alpha == 1.0:
        # no cross-entropy term: labels outside [0, C) are allowed and score no hit
        loss = distill_loss(logits, None, teacher_logits, temp, alpha)
        valid = (labels >= 0) & (labels < fc.out_features) & (soft[0] >= 0) & (soft[0] < fc.out_features)
    else:
        loss = F.cross_entropy(logits, soft_target(labels, soft[0], lam, smoothing, fc.out_features, logits.dtype))
        if len(soft) == 6:
            loss = distill_loss(logits, loss, teacher_logits, temp, alpha)
    with torch.no_grad():
        z = logits.detach()
        # the kernel's rank rule: a row hits@k when fewer than k logits exceed the label's
        if valid is None:
            above = (z > z.gather(1, labels[:, None])).sum(1)
        else:
            above = (z > z.gather(1, labels.clamp(0, fc.out_features - 1)[:, None])).sum(1)
            above = torch.where(valid, above, torch.full_like(above, fc.out_features))
        stats = torch.stack([loss.detach() * labels.numel(), (above < 1).sum().float(), (above < 5).sum().float()])
    return loss, stats.to(loss.dtype), logits.detach()


def classifier_ce(feat: torch.Tensor, fc: torch.nn.Linear, labels: torch.Tensor,
                  native: bool = True, gemm: str = "fma", labels2=None, lam: float = 1.0,
                  smoothing: float = 0.0, teacher_logits=None, temp: float = 1.0,
                  alpha: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(loss, stats)`` — see :func:`classifier_ce_logits`."""
    if teacher_logits is not None:
        loss, stats, _ = classifier_ce_logits(feat, fc, labels, native, gemm, labels2, lam, smoothing,
                                              teacher_logits, temp, alpha)
    elif labels2 is None and lam == 1.0 and smoothing == 0.0:
        loss, stats, _ = classifier_ce_logits(feat, fc, labels, native, gemm)      # today's call, as it was
    else:
        loss, stats, _ = classifier_ce_logits(feat, fc, labels, native, gemm, labels2, lam, smoothing)
    return loss, stats
