"""fp64 oracle of the encoder-to-loss path: global average pool (csrc/kernels/pool.hip), the
projection head (csrc/bindings/head_ops.cpp on the GEMMs of csrc/include/igemm_kernel.h, the cast
of csrc/kernels/head.hip, the column reduction of csrc/kernels/bn.hip) and the row normalisation /
norm statistics of csrc/kernels/featnorm.hip. Written from the definitions; it imports nothing of
the package. CPU tensors in, CPU float64 out.

Projection head (head_ops.cpp:6-14). With the inputs of tests/path_checks.py every partial sum is
exact in fp32 (the guard there), so a fp32 value is the real number and only the PLACE OF THE
ROUNDINGS is left to pin:

  fb  = bf16(feat)                cast_f32_bf16_kernel, head.hip:12-19 (pack8 -> v_cvt_pk_bf16_f32,
                                  round to nearest even, common.h:53-57); skipped for a bf16 feat
                                  (head_ops.cpp:85).
  h   = bf16(relu(fb·W1ᵀ + b1))   bias, then ReLU, on the fp32 accumulators (igemm_kernel.h:1169-1181),
                                  ONE rounding at the store (igemm_kernel.h:1249).
  z   = h·W2ᵀ + b2                the same bias epilogue, then the fp32 store straight from the
                                  accumulators (igemm_kernel.h:1183-1201): no bf16 rounding.
  dzb = bf16(dz)                  the cast kernel again (head_ops.cpp:183).
  db_last += Σ_rows dz            launch_col_reduce mode 3 over the fp32 dz viewed as a
                                  [rows][1][O] slab (head_ops.cpp:206): fp64 sums (bn.hip:195-199,
                                  208, 246, 255), ONE rounding to fp32 and a fp32 add into the sink
                                  (bn.hip:263). The fp32 dz, not dzb.
  dW2 += dzbᵀ·h                   fp32 split-K partial sums, summed in fp32 with the sink
                                  (tests/conv_oracle.py, "weight gradient").
  dh  = bf16(dzb·W2)·[h > 0]      rounded at igemm_kernel.h:1249, then masked by ya·1 + 0 > 0 on
                                  the bf16 h (igemm_kernel.h:1447; msc = 1, msh = 0 from
                                  head_ops.cpp:141-143) and stored masked (igemm_kernel.h:1453).
  db1 += Σ_rows dh                of the STORED bf16 values: the statistics unpack the packed bf16
                                  chunk (igemm_kernel.h:1440), mask it (1447) and add it (1456);
                                  per 64-row tile in fp32 (1456, 1477, 1492), the tiles in fp64 and
                                  one rounding into the sink (bn.hip:263). ``db1_acc`` below is the
                                  other reading (the fp32 accumulators), kept to show the cases
                                  tell the two apart.
  dW1 += dhᵀ·fb
  dfeat = dh·W1                   fp32 store (igemm_kernel.h:1183-1201).

Global average pool (pool.hip:163-195): y = fp32(fp32 Σ_hw x · fp32(1/HW)), the sum sequential in
pixel order (pool.hip:170-175), 1/HW one fp32 division (pool.hip:176); dx = bf16(fp32(dy·fp32(1/HW)))
(pool.hip:186, 192-193), the same value at every pixel.

Row normalisation (featnorm.hip:3-5): y = x / max(‖x‖, eps); dx = (dy − y·(y·dy)) / ‖x‖ where
‖x‖ > eps, dy / eps on the clamped rows (‖x‖ <= eps: featnorm.hip:67). Norm statistics
(featnorm.hip:6-10, 135-145): mean and variance of the row norms over the global rows, the
record_norm_mean EMA, loss_sec = Σ_local (‖x‖ − rec)² / n_global, loss_l2 = Σ_local ‖x‖² / n_global.
"""
from __future__ import annotations

import numpy as np
import torch

from conv_oracle import rne_bf16, trunc_bf16  # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------- projection head -------------

def head_fwd(feat, w1, b1, w2=None, b2=None):
    """feat [rows, D], w1 [O1, D], w2 [O2, O1] -> dict(fb, acc1, h, z); the single Linear: h None,
    z = fb·W1ᵀ + b1."""
    fb = rne_bf16(feat.to(F64))
    acc1 = fb @ w1.to(F64).T + b1.to(F64)
    if w2 is None:
        return dict(fb=fb, acc1=acc1, h=None, z=acc1)
    h = rne_bf16(acc1.clamp_min(0.0))
    return dict(fb=fb, acc1=acc1, h=h, z=h @ w2.to(F64).T + b2.to(F64))


def head_bwd(dz, fb, h, w1, w2=None):
    """The gradients (without the sinks) -> dict(dzb, db_last, dw1, dfeat[, dw2, dh_acc, dh, db1,
    db1_acc])."""
    dz = dz.to(F64)
    dzb = rne_bf16(dz)
    r = dict(dzb=dzb, db_last=dz.sum(0))
    if w2 is None:
        r.update(dw1=dzb.T @ fb, dfeat=dzb @ w1.to(F64))
        return r
    keep = (h > 0).to(F64)
    acc = dzb @ w2.to(F64)
    dh = rne_bf16(acc) * keep
    r.update(dw2=dzb.T @ h, dh_acc=acc, dh=dh, db1=dh.sum(0), db1_acc=(acc * keep).sum(0), dw1=dh.T @ fb,
             dfeat=dh @ w1.to(F64))
    return r


# ---------------------------------------------------------------- global average pool ---------

def inv_hw(HW):
    """fp32(1 / HW): one IEEE fp32 division."""
    return float(np.float32(1.0) / np.float32(HW))


def gap_fwd(x):
    """x [N, H, W, C] (bf16 values) -> (y, sabs): y = Σ_hw x · fp32(1/HW) in fp64, NOT rounded,
    sabs = Σ_hw |x|. Where Σ is exact in fp32 the kernel's value is y rounded once to fp32."""
    N, H, W, C = x.shape
    v = x.to(F64).reshape(N, H * W, C)
    return v.sum(1) * inv_hw(H * W), v.abs().sum(1)


def gap_bwd(dy, H, W):
    """dy [N, C] fp32 values -> dx [N, H, W, C]: the fp64 product of two fp32 values is exact, so
    its cast to fp32 is the kernel's single fp32 rounding; then bf16."""
    p = (dy.to(F64) * inv_hw(H * W)).to(F32).to(F64)
    return rne_bf16(p)[:, None, None, :].expand(dy.shape[0], H, W, dy.shape[1]).contiguous()


# ---------------------------------------------------------------- row normalisation -----------

def rownorm(x, eps):
    x = x.to(F64)
    n = (x * x).sum(1).sqrt()
    return x / n.clamp_min(eps)[:, None], n


def rownorm_bwd(dy, x, eps):
    y, n = rownorm(x, eps)
    dy = dy.to(F64)
    free = (dy - y * (y * dy).sum(1, keepdim=True)) / n.clamp_min(eps)[:, None]
    return torch.where((n > eps)[:, None], free, dy / eps)


def norm_sums(x):
    """-> (Σ‖x‖, Σ‖x‖², the row norms). The squares of a row are summed in ascending order, so
    rows that are signed permutations of each other get the same norm to the last bit."""
    n = (x.to(F64) ** 2).sort(1).values.sum(1).sqrt()
    return n.sum().item(), (n * n).sum().item(), n


def norm_finalize(n_local, g1, g2, n_global, momentum, rec):
    """rec: the EMA state before the call (None: not valid yet, the call ignores momentum).
    -> dict(mean, var, rec, sec, l2) as Python floats. var is the definition g2/n − mean²
    evaluated as the mean squared deviation where the local rows are all the rows."""
    mean = g1 / n_global
    var = g2 / n_global - mean * mean
    if abs(n_local.numel() - n_global) < 0.5:
        var = ((n_local - mean) ** 2).sum().item() / n_global
    r = mean if rec is None else (1.0 - momentum) * rec + momentum * mean
    return dict(mean=mean, var=var, rec=r, sec=((n_local - r) ** 2).sum().item() / n_global,
                l2=(n_local * n_local).sum().item() / n_global)
