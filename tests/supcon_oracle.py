"""fp64 oracle of the row-form contrastive loss (csrc/kernels/supcon.hip), independent of the
package: plain torch / numpy on the CPU.

Row form: anchor i has the contrast index ``self_idx[i]`` and the key ``akey[i]``; contrast j has
the key ``ckey[j]``; positive(i, j) <=> akey[i] == ckey[j] and j != self_idx[i].

  s_ij   = a_i·c_j / τ                         (j != self_idx[i])
  lse_i  = log Σ_j exp s_ij
  ℓ_i    = −(τ/τ_base)·(mean_{p∈P_i} s_ip − lse_i)          0 where P_i is empty
  loss   = scale·Σ_i ℓ_i
  G_ij   = w·g·(softmax_ij − pos_ij/|P_i|),  w = scale·(τ/τ_base)/τ     a zero row where P_i is empty
  dA_i   = Σ_j G_ij c_j          dC_j = Σ_i G_ij a_i

``exact`` evaluates this densely in fp64. ``split_model`` evaluates the arithmetic the kernel is
specified to do, with the roundings the specification names and no other: every fp32 input x is
hi = bf16_rne(x), lo = bf16_rne(x − hi); a product is hi·hi + hi·lo + lo·hi (the lo·lo term and
the remainder x − hi − lo are dropped); G is rounded to fp32 and split the same way for the
backward product. Everything else (sums, exp, log) is fp64.
"""
from __future__ import annotations

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64


def bf16_rne(x):
    """fp32 -> nearest bf16 (ties to even) as an fp32 tensor: what f2bf (csrc/include/common.h,
    the hardware conversion) returns. tests/test_supcon_oracle.py pins it to ``bf16_rne_int``."""
    return x.to(F32).bfloat16().to(F32)


def bf16_rne_int(x):
    """The same rounding in integer arithmetic on the bit pattern (finite inputs)."""
    b = x.to(F32).contiguous().numpy().view(np.uint32).astype(np.uint64)
    r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16) << np.uint64(16)
    return torch.from_numpy(r.astype(np.uint32).view(np.float32).copy()).reshape(x.shape)


def split(x):
    """-> (hi, lo) fp32 tensors; x − hi is exact in fp32 (hi keeps the leading 8 bits of x)."""
    x = x.to(F32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def masks(self_idx, akey, ckey, n):
    """-> (not_self, pos), both [Na, N] bool."""
    cols = torch.arange(n)
    not_self = cols[None, :] != self_idx.long()[:, None]
    return not_self, (akey.long()[:, None] == ckey.long()[None, :]) & not_self


def _loss_and_g(S, not_self, pos, tau, tau_base, scale, g):
    """Everything that follows from the fp64 logits S."""
    ninf = torch.full((), float("-inf"), dtype=F64)
    zero = torch.zeros((), dtype=F64)
    Sm = torch.where(not_self, S, ninf)
    m = Sm.max(1).values
    l = torch.exp(Sm - m[:, None]).sum(1)
    lse = m + torch.log(l)
    cnt = pos.sum(1)
    has = cnt > 0
    cd = cnt.clamp_min(1).to(F64)
    mean_pos = torch.where(pos, S, zero).sum(1) / cd
    ratio = tau / tau_base
    rows = torch.where(has, -ratio * (mean_pos - lse), zero)
    P = torch.exp(Sm - lse[:, None])                       # softmax; exactly 0 at self
    posw = pos.to(F64) / cd[:, None]
    w = scale * ratio / tau
    G = torch.where(has[:, None], (w * g) * (P - posw), zero)
    return dict(logits=S, not_self=not_self, pos=pos, max=m, lse=lse, cnt=cnt, has=has, mean_pos=mean_pos,
                rows=rows, loss=scale * rows.sum(), P=P, posw=posw, G=G, w=w)


def exact(A, C, self_idx, akey, ckey, tau, tau_base, scale, g=1.0):
    A, C = A.to(F64), C.to(F64)
    not_self, pos = masks(self_idx, akey, ckey, C.shape[0])
    o = _loss_and_g(A @ C.t() / tau, not_self, pos, tau, tau_base, scale, g)
    o["dA"] = o["G"] @ C
    o["dC"] = o["G"].t() @ A
    return o


def split_model(A, C, self_idx, akey, ckey, tau, tau_base, scale, g=1.0):
    Ah, Al = (t.to(F64) for t in split(A))
    Ch, Cl = (t.to(F64) for t in split(C))
    not_self, pos = masks(self_idx, akey, ckey, C.shape[0])
    S = (Ah @ Ch.t() + Ah @ Cl.t() + Al @ Ch.t()) / tau
    o = _loss_and_g(S, not_self, pos, tau, tau_base, scale, g)
    Gh, Gl = (t.to(F64) for t in split(o["G"].to(F32)))
    o["dA"] = Gh @ Ch + Gl @ Ch + Gh @ Cl
    o["dC"] = Gh.t() @ Ah + Gl.t() @ Ah + Gh.t() @ Al
    return o


def split_bound(A, C, tau):
    """|split_model logit − exact logit| <= (Σ_d |a_lo||c_lo| + |r_a||c| + |a||r_c|)/τ with r = x − hi − lo
    the remainder of the split: the header's "~2^-16" as an inequality (|a_lo| <= 2^-9|a| and
    |r| <= 2^-18|a| give 3·2^-18·Σ|a||c|/τ)."""
    Ah, Al = (t.to(F64) for t in split(A))
    Ch, Cl = (t.to(F64) for t in split(C))
    A, C = A.to(F64), C.to(F64)
    ra, rc = (A - Ah - Al).abs(), (C - Ch - Cl).abs()
    return (Al.abs() @ Cl.abs().t() + ra @ C.abs().t() + A.abs() @ rc.t()) / tau
