"""fp64 oracle of the convolution kernels (csrc/include/igemm_kernel.h, csrc/kernels/wgrad1x1.hip,
wgrad3x3.hip, splitk.hip), written from the definition in NHWC: explicit tap loops and a fp64
einsum, no call into torch's convolutions. CPU tensors in, CPU float64 out.

Layouts: x [N, H, W, C], w [K, R, S, C], y [N, P, Q, K], dy like y, the data gradient's weight
wt [C, R, S, K] (w with its ends swapped), dW [K, R, S, C].

The kernels multiply bf16 operands and accumulate in fp32. The inputs of tests/conv_checks.py
are small integers and dyadic fractions chosen so that every partial sum, in any order, is
exact in fp32 (the guard there); what is left to pin is the ORDER OF THE ROUNDINGS, taken from
the epilogue of igemm_kernel.h:

  operand prologue   a = bf16(relu(x·s + t)), fp32 math and ONE rounding (bnrelu8, lines
                     180-189); applied to loaded taps only, so a pad tap stays 0 and is not
                     relu(t) (ld_mask, lines 740-745). Forward: the x operand; weight gradient:
                     the x operand.
  forward            acc -> [+ bias, then ReLU, on the accumulators: lines 1169-1182]
                     -> bf16 (line 1249). The statistics Σy, Σy² are taken from the fp32
                     ACCUMULATORS, not from the stored values (lines 1499-1538); the binding
                     never asks for them together with the bias epilogue.
  data gradient      acc -> [+ bias_pre, fp32, the K-concatenated form: lines 1204-1220]
                     -> bf16 (line 1249) -> [+ addend: bf16(bf16(acc) + addend·bit), a SECOND
                     rounding, lines 1391-1412]. The bindings never set add_pre, so the addend
                     always joins after the first rounding (has_add, line 1260). A compact
                     addend (addend_sub = s) is read at pixels with h, w ≡ 0 mod s only (lines
                     1292-1298).
  BN-backward sums   of the STORED dx, i.e. after both roundings (lines 1437-1465): d = dx·m
                     with m from the bitmask (line 1444), from ya·msc + msh > 0 in fp32 (line
                     1447) or absent; Σd, Σd·(ya − μa), Σd·(yb − μb) with fmaf. store_masked
                     (VAR 2, line 1453) stores d in place of dx. An empty ya counts as 0
                     (lines 1318-1321).
  weight gradient    fp32 partial sums per split stored unrounded (lines 1183-1201), summed in
                     fp32 by splitk.hip, + the sink when accumulating.

With exact partial sums a fp32 value is the real number, so the oracle works on reals in
float64 and rounds where the kernel rounds, with ``rne_bf16``.
"""
from __future__ import annotations

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64


def _f32_pattern(t64: torch.Tensor) -> np.ndarray:
    f = t64.to(F64).to(F32)
    assert torch.equal(f.to(F64), t64.to(F64)), "rne_bf16: the value is not a float32 (the guard failed?)"
    return f.contiguous().numpy().view(np.uint32).astype(np.uint64)


def _from_pattern(u: np.ndarray, shape) -> torch.Tensor:
    return torch.from_numpy(u.astype(np.uint32).view(np.float32).copy()).reshape(shape).to(F64)


def rne_bf16(t64: torch.Tensor) -> torch.Tensor:
    """Round float32-representable values to bf16, nearest-even, as an integer operation on the
    fp32 pattern: add 0x7fff plus the lowest kept bit, clear the low half. (Finite values.)"""
    u = _f32_pattern(t64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return _from_pattern(u, t64.shape)


def trunc_bf16(t64: torch.Tensor) -> torch.Tensor:
    """The deliberate defect: the low half cleared without rounding."""
    return _from_pattern(_f32_pattern(t64) & np.uint64(0xFFFF0000), t64.shape)


def out_size(H, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1


def prologue(x, scale, shift):
    """bf16(relu(x·s + t)) per channel, one rounding."""
    return rne_bf16((x.to(F64) * scale.to(F64) + shift.to(F64)).clamp_min(0.0))


def patches(x, R, S, stride, pad):
    """[N, H, W, C] -> [N, P, Q, R, S, C]: tap (r, s) of output pixel (p, q) is input pixel
    (p·stride − pad + r, q·stride − pad + s), zero outside the image."""
    x = x.to(F64)
    N, H, W, C = x.shape
    P, Q = out_size(H, R, stride, pad), out_size(W, S, stride, pad)
    xp = torch.zeros(N, H + 2 * pad + stride, W + 2 * pad + stride, C, dtype=F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = torch.empty(N, P, Q, R, S, C, dtype=F64)
    for r in range(R):
        for s in range(S):
            cols[:, :, :, r, s] = xp[:, r:r + stride * P:stride, s:s + stride * Q:stride][:, :P, :Q]
    return cols


def fwd_acc(x, w, stride, pad, in_scale=None, in_shift=None):
    """The accumulators [N, P, Q, K]."""
    a = x.to(F64) if in_scale is None else prologue(x, in_scale, in_shift)
    K, R, S, C = w.shape
    return torch.einsum("npqrsc,krsc->npqk", patches(a, R, S, stride, pad), w.to(F64))


def fwd(x, w, stride, pad, in_scale=None, in_shift=None, bias=None, relu=False):
    """-> dict(acc, y, sums [2, K]): y the stored bf16 values; sums = Σ, Σ² of the accumulators
    over the pixels (before the bias epilogue, which runs without statistics)."""
    acc = fwd_acc(x, w, stride, pad, in_scale, in_shift)
    rows = acc.reshape(-1, acc.shape[-1])
    v = acc
    if bias is not None:
        v = v + bias.to(F64)
    if relu:
        v = v.clamp_min(0.0)
    return dict(acc=acc, y=rne_bf16(v), sums=torch.stack([rows.sum(0), (rows * rows).sum(0)]))


def tile_rows(rows, bm):
    """[M, C] -> [ceil(M / bm), C]: the sums of rows [mt·bm, (mt+1)·bm)."""
    M, C = rows.shape
    mt = -(-M // bm)
    pad = torch.zeros(mt * bm, C, dtype=F64)
    pad[:M] = rows
    return pad.reshape(mt, bm, C).sum(1)


def dgrad_acc(dy, wt, H, W, stride, pad):
    """dx[n, h, w, c] = Σ dy[n, p, q, k]·wt[c, r, s, k] over (p, q, r, s) with
    h = p·stride − pad + r, w = q·stride − pad + s: each tap scattered onto its pixels."""
    dy, wt = dy.to(F64), wt.to(F64)
    N, P, Q, K = dy.shape
    C, R, S, _ = wt.shape
    dxp = torch.zeros(N, H + 2 * pad + stride + R, W + 2 * pad + stride + S, C, dtype=F64)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + stride * P:stride, s:s + stride * Q:stride][:, :P, :Q] += \
                torch.einsum("npqk,ck->npqc", dy, wt[:, r, s, :])
    return dxp[:, pad:pad + H, pad:pad + W].contiguous()


def unpack_bits(bits, shape):
    """Packed uint8 (bit i of byte e: element 8e + i) -> float64 0/1 tensor of ``shape``."""
    b = bits.numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(b.astype(np.uint8), bitorder="little")[:n].astype(np.float64)).reshape(shape)


def pack_bits(keep):
    return torch.from_numpy(np.packbits(keep.reshape(-1).numpy().astype(bool), bitorder="little"))


def expand_addend(addend, bits, sub, shape):
    """The addend as a full [N, H, W, C] float64 tensor: masked by its bits, or a compact
    [N, ceil(H/s), ceil(W/s), C] tensor placed at h, w ≡ 0 mod s (zero elsewhere)."""
    a = addend.to(F64)
    if sub > 1:
        full = torch.zeros(shape, dtype=F64)
        full[:, ::sub, ::sub] = a
        return full
    return a * unpack_bits(bits, shape) if bits is not None else a


def dgrad(dy, wt, H, W, stride, pad, addend=None, addend_bits=None, addend_sub=0, cat=None, cat_bias=None,
          round1=rne_bf16):
    """The stored dx. cat / cat_bias: wt is [C, 1, 1, K + K2] and the reduction runs over
    [dy | cat], with the fp32 bias joining before the rounding."""
    if cat is not None:
        K = dy.shape[-1]
        acc = dgrad_acc(dy, wt[..., :K], H, W, 1, 0) + dgrad_acc(cat, wt[..., K:], H, W, 1, 0) + cat_bias.to(F64)
    else:
        acc = dgrad_acc(dy, wt, H, W, stride, pad)
    dx = round1(acc)
    if addend is not None:
        dx = round1(dx + expand_addend(addend, addend_bits, addend_sub, dx.shape))
    return dx


def bn_mask(shape, mask, ya):
    """mask: None | ("bits", uint8) | ("affine", msc, msh) -> float64 0/1 or None."""
    if mask is None:
        return None
    if mask[0] == "bits":
        return unpack_bits(mask[1], shape)
    return (ya.to(F64) * mask[1].to(F64) + mask[2].to(F64) > 0).to(F64)


def bn_terms(dx, mask, ya, ma, yb=None, mb=None):
    """-> (d, terms [2|3, M, C]): d = dx·m and the per-pixel terms d, d·(ya − μa), d·(yb − μb);
    ya None: 0."""
    m = bn_mask(dx.shape, mask, ya)
    d = dx if m is None else dx * m
    C = dx.shape[-1]
    y0 = torch.zeros_like(dx) if ya is None else ya.to(F64)
    t = [d, d * (y0 - ma.to(F64))]
    if yb is not None:
        t.append(d * (yb.to(F64) - mb.to(F64)))
    return d, torch.stack([v.reshape(-1, C) for v in t])


def wgrad(dy, x, R, S, stride, pad, in_scale=None, in_shift=None, sink=None, pixels=None):
    """dW[k, r, s, c] = Σ dy[n, p, q, k]·x[n, p·stride − pad + r, q·stride − pad + s, c]
    (+ sink); pixels: a (begin, end) range of the flattened (n, p, q) index, one split's share."""
    a = x.to(F64) if in_scale is None else prologue(x, in_scale, in_shift)
    cols = patches(a, R, S, stride, pad)
    K = dy.shape[-1]
    d2, c2 = dy.to(F64).reshape(-1, K), cols.reshape(-1, R, S, cols.shape[-1])
    if pixels is not None:
        d2, c2 = d2[pixels[0]:pixels[1]], c2[pixels[0]:pixels[1]]
    dw = torch.einsum("mk,mrsc->krsc", d2, c2)
    return dw if sink is None else dw + sink.to(F64)
