"""fp64 definitions of Mixup / CutMix and the soft-target cross-entropy, written from their
specification and not from the kernels (csrc/kernels/mix.hip, csrc/include/soft_ce.h).

Mixing (batch mode): the partner of batch row i is row (i − 1) mod B.
    CutMix  out[i] = x[i−1] inside the box [y0, y1) x [x0, x1), x[i] outside.
    Mixup   s[i] = w0·x[i] + w1·x[i−1] in exact arithmetic (fp64 holds the sum of two products of
            an fp32 weight and a bf16 value exactly: 24 + 8 significant bits each, and the
            exponents of the tests' values are close), rounded ONCE to bf16, nearest even.
            The weights are inputs: w0 = fp32(λ), w1 = fp32(1 − w0).
Box (torchvision v2 CutMix, square image of side S, centre (cy, cx) uniform over the pixels):
    half = trunc(0.5·sqrt(1 − λ)·S); y0 = max(cy − half, 0), y1 = min(cy + half, S), x alike;
    λ' = 1 − (y1 − y0)(x1 − x0) / S².
Soft target of a row with labels a, b:  t_c = (1 − ε)(λ[c = a] + (1 − λ)[c = b]) + ε/C
    loss = lse(z) − Σ_c t_c z_c,  dz = (softmax(z) − t)·gscale,  hit@k: #{z_c > z_a} < k.
    A row with either label outside [0, C): loss NaN, no hit, dz = softmax·gscale.
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64


def partner(x: torch.Tensor) -> torch.Tensor:
    B = x.shape[0]
    return x[[(i - 1) % B for i in range(B)]]


def cutmix(x: torch.Tensor, box) -> torch.Tensor:
    """x [B, H, W, C] of any dtype: a bit copy."""
    y0, y1, x0, x1 = box
    H, W = x.shape[1], x.shape[2]
    yy = torch.arange(H).view(1, H, 1, 1)
    xx = torch.arange(W).view(1, 1, W, 1)
    inside = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
    return torch.where(inside, partner(x), x)


def mixup_weights(lam: float):
    w0 = torch.tensor(lam, dtype=torch.float32)
    w1 = torch.tensor(1.0, dtype=torch.float32) - w0
    return float(w0), float(w1)


def mixup_exact(x: torch.Tensor, lam: float) -> torch.Tensor:
    """The unrounded fp64 value w0·x[i] + w1·x[i−1] of bf16 (or any) x."""
    w0, w1 = mixup_weights(lam)
    return w0 * x.to(F64) + w1 * partner(x).to(F64)


def round_bf16(s: torch.Tensor) -> torch.Tensor:
    """fp64 -> bf16, round to nearest even, in integers (no intermediate fp32 rounding)."""
    m, e = torch.frexp(s)                          # s = m·2^e, 0.5 <= |m| < 1
    q = torch.round(m * 256.0)                     # 8 significant bits; torch.round is half-to-even
    return torch.ldexp(q, e - 8).to(torch.bfloat16)   # (exact: q·2^(e−8) has <= 9 bits)


def box_rule(lam: float, cy: int, cx: int, S: int):
    half = math.trunc(0.5 * math.sqrt(1.0 - lam) * S)
    y0, y1 = max(cy - half, 0), min(cy + half, S)
    x0, x1 = max(cx - half, 0), min(cx + half, S)
    return (y0, y1, x0, x1), 1.0 - ((y1 - y0) * (x1 - x0)) / float(S * S)


def soft_target(a, b, lam: float, eps: float, C: int) -> torch.Tensor:
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    t = torch.zeros(a.numel(), C, dtype=F64)
    for r in range(a.numel()):
        t[r, int(a[r])] += (1.0 - eps) * lam
        t[r, int(b[r])] += (1.0 - eps) * (1.0 - lam)
    return t + eps / C


def soft_ce(z: torch.Tensor, a, b, lam: float, eps: float, gscale: float):
    """z [B, C] -> dict(loss [B], dz [B, C], hit1 [B], hit5 [B], lse, p, t, ok), all fp64."""
    z = z.to(F64)
    B, C = z.shape
    a, b = torch.as_tensor(a).long().cpu(), torch.as_tensor(b).long().cpu()
    ok = (a >= 0) & (a < C) & (b >= 0) & (b < C)
    m = z.max(1).values
    lse = m + torch.log(torch.exp(z - m[:, None]).sum(1))
    p = torch.exp(z - lse[:, None])
    t = torch.zeros(B, C, dtype=F64)
    t[ok] = soft_target(a[ok], b[ok], lam, eps, C)
    loss = lse - (t * z).sum(1)
    loss[~ok] = float("nan")
    za = z.gather(1, a.clamp(0, C - 1)[:, None])
    above = (z > za).sum(1)
    return dict(loss=loss, dz=(p - t) * gscale, hit1=(ok & (above < 1)).to(F64), hit5=(ok & (above < 5)).to(F64),
                lse=lse, p=p, t=t, ok=ok, m=m)
