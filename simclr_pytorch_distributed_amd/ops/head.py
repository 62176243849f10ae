"""Projection head (reference networks/resnet_big.py:159-181: MLP Linear-ReLU-Linear or a
single Linear) as ONE autograd node on the native path.

Both directions are one host call into the C++ head executor (csrc/bindings/head_ops.cpp),
which runs the GEMMs as 1x1 implicit GEMMs of the hand-written MFMA kernel (igemm.hip)
with fused epilogues: bias + ReLU on the fp32 accumulators, fp32 feature output, ReLU
backward fused into the hidden-gradient store together with its column sums (the hidden
bias gradient). Weight and bias gradients are accumulated straight into the parameter
sinks. The bf16 weights come from the per-step weight cache (ops/weights.py caches the
head's Linear layers as 1x1 convs, in both the forward and the transposed layout).
Numerics: bf16 operands, fp32 accumulation, fp32 biases, bf16 hidden activation, fp32
output — the reference computed under autocast, with the bias added before rounding.

The BatchNorm projector (``--head mlp_bn``: Linear -> BatchNorm1d -> ReLU hidden layers, models/resnet.py
``bn_projector``) is one node as well (``_BNHead``, csrc/bindings/head_bn_ops.cpp): every hidden layer
is ONE launch per direction of the column-strip-owned kernels of csrc/kernels/head_bn.hip (GEMM +
batch statistics + normalise + ReLU; BN + ReLU backward with the γ / β gradients), the last Linear
and the weight / data gradients run on the GEMMs above. Kept for backward per hidden layer: the bf16
pre-activation and μ, rstd; the activation is recomputed. Outside the kernels' range (2 <= rows <=
2048, in = 64j <= 8192, hidden = 32j <= 8192), in eval mode and with a SyncBatchNorm head the modules
run instead (``models/executor.py head_forward``), with one warning.
"""
from __future__ import annotations

import logging
import os

import torch

from . import _ext, sinks


_HEAD_SIDE = os.environ.get("SDX_HEAD_SIDE", "1") != "0"


def _side(t: torch.Tensor) -> int:
    """the wgrad side stream's handle for the head's weight gradients (0: none). The current
    backward pass then ends with a join (compute stream behind the side stream), so the
    parameter gradients are complete for whatever runs after ``backward()`` on the compute
    stream, not only for the optimizer step (which joins as well)."""
    from . import streams
    if not (_HEAD_SIDE and streams.ENABLED and t.is_cuda):
        return 0
    dev = t.device
    main, side = torch.cuda.current_stream(dev), streams.side(dev)   # (this node's stream)

    def _join():
        main.wait_stream(side)
        streams.release()

    torch.autograd.Variable._execution_engine.queue_callback(_join)
    return side.cuda_stream


class _MLPHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, w1b, w2b, w1t, w2t, l1, l2, *params):
        z, fb, h = _ext.require().head_fwd(feat, w1b, l1.bias.detach(), w2b, l2.bias.detach())
        ctx.save_for_backward(fb, h, w1t, w2t)
        ctx.mods = (l1, l2)
        ctx.params = params
        ctx.feat_dtype = feat.dtype
        return z

    @staticmethod
    def backward(ctx, dz):
        fb, h, w1t, w2t = ctx.saved_tensors
        l1, l2 = ctx.mods
        t = sinks.target
        dfeat = _ext.require().head_bwd(dz.float(), fb, h, w1t, w2t, t(l1.weight), t(l1.bias), t(l2.weight),
                                        t(l2.bias), _side(dz))
        sinks.notify(ctx.params)
        return (dfeat.to(ctx.feat_dtype), None, None, None, None, None, None) + (None,) * len(ctx.params)


class _LinearHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, wb, wt, lin, *params):
        z, fb, _ = _ext.require().head_fwd(feat, wb, lin.bias.detach())
        ctx.save_for_backward(fb, wt)
        ctx.lin = lin
        ctx.params = params
        ctx.feat_dtype = feat.dtype
        return z

    @staticmethod
    def backward(ctx, dz):
        fb, wt = ctx.saved_tensors
        lin = ctx.lin
        dfeat = _ext.require().head_bwd(dz.float(), fb, None, wt, None, sinks.target(lin.weight),
                                        sinks.target(lin.bias))
        sinks.notify(ctx.params)
        return (dfeat.to(ctx.feat_dtype), None, None, None) + (None,) * len(ctx.params)


def _w(wc, lin) -> torch.Tensor:
    return wc.fwd(lin).view(lin.out_features, lin.in_features)


def _wt(wc, lin) -> torch.Tensor:
    return wc.dgrad(lin).view(lin.in_features, lin.out_features)


class _BNHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, head, *rest):
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        bns = [m for m in head if isinstance(m, torch.nn.BatchNorm1d)]
        L = len(lins)
        wbs, wts, params = list(rest[:L]), list(rest[L:2 * L]), rest[2 * L:]
        out = _ext.require().head_bn_fwd(feat, wbs, [b.weight.detach() for b in bns], [b.bias.detach() for b in bns],
                                         [b.running_mean for b in bns], [b.running_var for b in bns],
                                         bns[0].momentum, bns[0].eps)
        ctx.save_for_backward(*out[1:], *wts)       # fb, then (yb, mu, rstd) per hidden layer
        ctx.mods = (lins, bns)
        ctx.params = params
        ctx.feat_dtype = feat.dtype
        return out[0]

    @staticmethod
    def backward(ctx, dz):
        lins, bns = ctx.mods
        L = len(lins)
        saved = ctx.saved_tensors
        fb, per, wts = saved[0], saved[1:1 + 3 * (L - 1)], list(saved[1 + 3 * (L - 1):])
        t = sinks.target
        dfeat = _ext.require().head_bn_bwd(dz.float(), fb, list(per[0::3]), list(per[1::3]), list(per[2::3]),
                                           [b.weight.detach() for b in bns], [b.bias.detach() for b in bns], wts,
                                           [t(l.weight) for l in lins], [t(b.weight) for b in bns],
                                           [t(b.bias) for b in bns], _side(dz))
        sinks.notify(ctx.params)
        return (dfeat.to(ctx.feat_dtype), None) + (None,) * (2 * L + len(ctx.params))


_bn_head_warned = False


def bn_head_native(head, feat: torch.Tensor) -> bool:
    """Can ``head`` (a ``bn_projector``) run on the head_bn kernels for these features? The reason why
    not is logged once."""
    global _bn_head_warned
    bns = [m for m in head if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    lins = [m for m in head if isinstance(m, torch.nn.Linear)]
    why = None
    if not head.training:
        return False                    # evaluation: the modules, silently (running statistics)
    if not all(type(b) is torch.nn.BatchNorm1d for b in bns):
        why = "its BatchNorms are synchronised"
    elif not all(b.affine and b.track_running_stats and b.momentum == bns[0].momentum and b.eps == bns[0].eps
                 and b.momentum is not None for b in bns):
        why = "its BatchNorms differ from affine BatchNorm1d with one momentum and eps"
    elif not (feat.is_cuda and _ext.require().head_bn_supported(feat.shape[0], lins[0].in_features,
                                                                lins[0].out_features, len(lins))):
        why = (f"{feat.shape[0]} rows, {lins[0].in_features} -> {lins[0].out_features} is outside the kernels' range "
               "(2 <= rows <= 2048, in = 64j <= 8192, hidden = 32j <= 8192)")
    if why is not None and not _bn_head_warned:
        _bn_head_warned = True
        logging.warning(f"mlp_bn head: running as torch modules: {why}")
    return why is None


def projection_head(feat: torch.Tensor, head, wc) -> torch.Tensor:
    """``head(feat)`` in bf16 with fp32 output, as one autograd node."""
    from ..models.resnet import is_bn_projector
    if is_bn_projector(head):
        if not bn_head_native(head, feat):
            from ..models.executor import head_forward
            return head_forward(head, feat)
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        params = [p for m in head for p in m.parameters(recurse=False)]
        return _BNHead.apply(feat, head, *[_w(wc, l) for l in lins], *[_wt(wc, l) for l in lins], *params)
    if isinstance(head, torch.nn.Linear):
        return _LinearHead.apply(feat, _w(wc, head), _wt(wc, head), head, head.weight, head.bias)
    l1, l2 = head[0], head[2]
    return _MLPHead.apply(feat, _w(wc, l1), _w(wc, l2), _wt(wc, l1), _wt(wc, l2), l1, l2, l1.weight, l1.bias,
                          l2.weight, l2.bias)
