"""fp64 definition of the knowledge-distillation loss of the supervised trainer (--distill_ckpt),
written from its specification and not from the kernels (csrc/include/distill_ce.h).

For a row with student logits z, teacher logits v, labels a, b and the soft target t of
``mix_oracle`` (t_c = (1 − ε)(λ[c = a] + (1 − λ)[c = b]) + ε/C):
    p = softmax(z),  q_s = softmax(z·it),  q_t = softmax(v·it)
    ce   = lse(z) − Σ_c t_c z_c
    kd   = τ²·KL(q_t ‖ q_s) = τ²·(Σ_c q_t,c·(v_c − z_c)·it − lse(v·it) + lse(z·it))
    loss = (1 − α)·ce + α·kd
    dz   = ((1 − α)·(p − t) + α·τ·(q_s − q_t))·gscale
    hit@k: #{z_c > z_a} < k   (the student's logits against label a)
``it`` and ``tau`` are inputs — the fp32 values the kernel receives (it = fp32(1/τ)) — and every
operation on them is fp64.
Rules: 0 <= α < 1 and a label outside [0, C): loss NaN, no hit, dz without the target term.
α = 1: the ce term is not formed; such a row is valid, its loss is kd, and it scores no hit.
"""
from __future__ import annotations

import torch

import mix_oracle as MO

F64 = torch.float64
F32 = torch.float32


def f32(v) -> float:
    return float(torch.tensor(v, dtype=F32))


def temperature(temp: float):
    """(it, tau) as the launchers make them: tau = fp32(temp), it = the fp32 quotient 1 / tau."""
    tau = torch.tensor(temp, dtype=F32)
    return float(torch.tensor(1.0, dtype=F32) / tau), float(tau)


def softmax64(x: torch.Tensor):
    """fp64 x [B, C] -> dict(m, lse, p), the shape ``mix_checks.softmax_stage_bounds`` takes."""
    m = x.max(1).values
    lse = m + torch.log(torch.exp(x - m[:, None]).sum(1))
    return dict(m=m, lse=lse, p=torch.exp(x - lse[:, None]))


def distill_ce(z, v, a, b, lam: float, eps: float, it: float, tau: float, alpha: float, gscale: float):
    """z, v [B, C] -> dict(loss [B], dz [B, C], hit1, hit5, ce, kd, valid, S (soft_ce of z), Qs, Qt), fp64."""
    z, v = z.to(F64).cpu(), v.to(F64).cpu()
    S = MO.soft_ce(z, a, b, lam, eps, 1.0)
    Qs, Qt = softmax64(z * it), softmax64(v * it)
    kd = tau * tau * ((Qt["p"] * ((v - z) * it)).sum(1) - Qt["lse"] + Qs["lse"])
    g = alpha * tau * (Qs["p"] - Qt["p"])
    if alpha == 1.0:
        loss, valid = alpha * kd, torch.ones_like(S["ok"])
    else:
        loss, valid = (1.0 - alpha) * S["loss"] + alpha * kd, S["ok"]
        g = (1.0 - alpha) * S["dz"] + g
    return dict(loss=loss, dz=g * gscale, hit1=S["hit1"], hit5=S["hit5"], ce=S["loss"], kd=kd, valid=valid, S=S,
                Qs=Qs, Qt=Qt)
