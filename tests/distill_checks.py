"""Cases, derived bounds, an fp32 twin and the comparison for the distillation row routine
(csrc/include/distill_ce.h) against ``distill_oracle``. The same check runs on the twin (CPU,
tests/test_distill_oracle.py, where every named defect must be caught) and on the kernels
(tests/test_gpu_distill.py). u = 2^-24; every bound is derived here, none is measured.

The reference is the fp64 oracle on the implementation's OWN logits z and the teacher's logits v
(the logits are the plain ops' bit for bit; their accuracy is the plain tests' subject).

Three softmaxes. ``mix_checks.softmax_stage_bounds`` bounds one fp32 softmax of EXACT inputs x in
the kernels' expressions and order: B_lse(x) on the lse, Δp_c(x) on every probability. It is applied
to z, to z·it and to v·it. The last two inputs are themselves rounded products, x~_c = fl(x_c·it)
with |x~_c − x_c| <= u|x_c·it|; a perturbation δ_c of the inputs moves the lse by at most
max_c|δ_c| and a probability by the factor exp(δ_c − Δlse):
    P(x)     = u·max_c|x_c|                                     (x the scaled row)
    B_lse'   = B_lse(x) + P(x)
    Δq_c     = Δp_c(x) + q_c·(u|x_c| + P(x))·SECOND_ORDER
(the scaled maximum fl(m·it) is max_c x~_c exactly: rounding is monotone and it > 0).

kd = fl(t2·fl(fl(kl − lse_t) + lse_s)), t2 = fl(τ·τ), kl = Σ_c fl(q_t,c·fl(fl(v_c − z_c)·it)) in fp32
through n_add = ceil(C/64) + 6 additions (lane partial sums in index order, then 6 shuffle steps);
with x_c = (v_c − z_c)·it:
    B_kl   = Σ_c (Δq_t,c·|x_c| + 3u·q_t,c|x_c|)·SECOND_ORDER          (q_t, the two roundings of x_c, the
             + n_add·u·Σ_c q_t,c|x_c|·SECOND_ORDER                     product: fused or not; the additions)
    B_in   = B_kl + B_lse'(v·it) + u|kl − lse_t| + B_lse'(z·it) + u|inner|
    B_kd   = τ²·B_in·SECOND_ORDER + 2u|kd|                              (t2 and the product)
The blend, ca = fl(1 − α):
    B_loss = (1 − α)·B_ce + α·B_kd + 2u|(1 − α)·ce| + u|α·kd| + u|loss|
with B_ce = ``mix_checks.soft_bounds``' row bound; at α = 1 the ce terms vanish (no ce is formed).
dz_c = fl(fl(fl(ca·fl(p_c − t_c)) + fl(ck·fl(q_s,c − q_t,c)))·gscale), ck = fl(α·τ):
    B_dz = gscale·((1 − α)·(Δp_c + Δt_c + u|p_c − t_c|) + 2u(1 − α)|p_c − t_c|
                   + α·τ·(Δq_s,c + Δq_t,c + u|q_s,c − q_t,c|) + 2u·α·τ|q_s,c − q_t,c|
                   + u|d_c|)·SECOND_ORDER + u|dz_c| + FTZ
where d_c = dz_c / gscale, Δt_c is soft_bounds' target term and FTZ = 2^-126 is the flush of a result
below the smallest normal number (Δp, Δq carry their own). Hits follow the rank rule on z exactly.
"""
from __future__ import annotations

import math

import torch

import distill_oracle as DO
import mix_checks as MC

F32, F64 = torch.float32, torch.float64
U, SECOND_ORDER, FTZ = MC.U, MC.SECOND_ORDER, MC.FTZ

DEFECTS = ("no_tau2", "no_tau_dz", "kl_swapped", "ce_at_alpha1", "temp_on_hard", "hits_teacher")
TEACHERS = ("equal", "perm", "peaky", "const", "random")


def teacher_rows(z: torch.Tensor, kind: str, seed: int = 0) -> torch.Tensor:
    """Teacher logits [B, C] (fp32) for student logits z: the student's own row, a permutation of it,
    ±40 entries (one-hot-like distributions and exponent underflow at τ < 1), a constant row (the
    uniform distribution), Gaussian rows."""
    z = z.to(F32).cpu()
    B, C = z.shape
    g = torch.Generator().manual_seed(7919 * B + 13 * C + seed)
    if kind == "equal":
        return z.clone()
    if kind == "perm":
        return torch.stack([z[r][torch.randperm(C, generator=g)] for r in range(B)])
    if kind == "peaky":
        return torch.where(torch.rand(B, C, generator=g) < 0.5, -40.0, 40.0).to(F32)
    if kind == "const":
        return torch.full((B, C), 1.5, dtype=F32)
    if kind == "random":
        return 3.0 * torch.randn(B, C, generator=g)
    raise ValueError(kind)


def _scaled_stage(x64, Q):
    """B_lse', Δq of the module docstring for the scaled row x64 = (logits·it) in fp64."""
    B_lse, dp, n_add = MC.softmax_stage_bounds(x64, Q)
    P = U * x64.abs().max(1).values
    dq = dp + Q["p"] * (U * x64.abs() + P[:, None]) * SECOND_ORDER
    return B_lse + P, dq, n_add


def distill_bounds(z, v, a, b, lam, eps, it, tau, alpha, gscale):
    """z: the implementation's logits, v: the teacher's (fp32) -> dict(ref = oracle, row, dz)."""
    z, v = z.to(F64).cpu(), v.to(F64).cpu()
    lam, eps, alpha = DO.f32(lam), DO.f32(eps), DO.f32(alpha)
    R = DO.distill_ce(z, v, a, b, lam, eps, it, tau, alpha, gscale)
    S, Qs, Qt = R["S"], R["Qs"], R["Qt"]
    _, dp, _ = MC.softmax_stage_bounds(z, S)
    SB = MC.soft_bounds(z, a, b, lam, eps, 1.0)
    Bs, dqs, n_add = _scaled_stage(z * it, Qs)
    Bt, dqt, _ = _scaled_stage(v * it, Qt)
    x = ((v - z) * it).abs()
    qx = Qt["p"] * x
    kl = (Qt["p"] * ((v - z) * it)).sum(1)
    B_kl = ((dqt * x + 3 * U * qx).sum(1) + n_add * U * qx.sum(1)) * SECOND_ORDER
    inner = kl - Qt["lse"] + Qs["lse"]
    B_in = B_kl + Bt + U * (kl - Qt["lse"]).abs() + Bs + U * inner.abs()
    B_kd = tau * tau * B_in * SECOND_ORDER + 2 * U * R["kd"].abs()
    ca, ck = 1.0 - alpha, alpha * tau
    ce = R["ce"].nan_to_num(0.0)
    loss = R["loss"].nan_to_num(0.0)
    row = alpha * B_kd + U * (alpha * R["kd"]).abs() + U * loss.abs()
    if alpha != 1.0:
        row = row + ca * SB["row"] + 2 * U * (ca * ce).abs()
    pt = (S["p"] - S["t"]).abs()
    qq = (Qs["p"] - Qt["p"]).abs()
    d = R["dz"] / gscale
    inner_dz = ck * (dqs + dqt + U * qq) + 2 * U * ck * qq + U * d.abs()
    if alpha != 1.0:
        inner_dz = inner_dz + ca * (dp + SB["dt"] + U * pt) + 2 * U * ca * pt
    dz = gscale * inner_dz * SECOND_ORDER + U * R["dz"].abs() + FTZ
    return dict(ref=R, row=row, dz=dz)


def check_distill(worst, ctx, z, v, a, b, lam, eps, temp, alpha, gscale, rowstat, dz):
    """rowstat [B, 3], dz [B, C] of an implementation whose logits are z, teacher logits v. Every row
    loss and every element of dz against its own bound; the worst error / bound goes to ``worst``."""
    it, tau = DO.temperature(temp)
    Bd = distill_bounds(z, v, a, b, lam, eps, it, tau, alpha, gscale)
    R = Bd["ref"]
    rs, dz = rowstat.to(F64).cpu(), dz.to(F64).cpu()
    ok = R["valid"]
    assert bool(torch.isnan(rs[~ok, 0]).all()) and not bool(torch.isnan(rs[ok, 0]).any()), f"{ctx}: NaN rows"
    assert torch.equal(rs[:, 1], R["hit1"]) and torch.equal(rs[:, 2], R["hit5"]), f"{ctx}: hits"
    el = (rs[ok, 0] - R["loss"][ok]).abs()
    ed = (dz - R["dz"]).abs()
    assert not bool(torch.isnan(ed).any()), f"{ctx}: NaN in dz"
    if el.numel():
        r = float((el / Bd["row"][ok]).max())
        worst.see(r, f"{ctx} loss")
        assert r <= 1.0, f"{ctx}: row loss error / bound {r:.3f}"
    r = float((ed / Bd["dz"]).max())
    worst.see(r, f"{ctx} dz")
    assert r <= 1.0, f"{ctx}: dz error / bound {r:.3f}"


def distill_twin(z, v, a, b, lam, eps, temp, alpha, gscale, defect=None):
    """fp32 torch twin of distill_ce_row on logits z, teacher v -> (rowstat [B, 3], dz [B, C])."""
    z, v = z.to(F32).cpu(), v.to(F32).cpu()
    B, C = z.shape
    a, b = torch.as_tensor(a).long().cpu(), torch.as_tensor(b).long().cpu()
    ok = (a >= 0) & (a < C) & (b >= 0) & (b < C)
    t32 = lambda x: torch.tensor(x, dtype=F32)      # noqa: E731
    tau = t32(temp)
    it = t32(1.0) / tau
    al, gs = t32(alpha), t32(gscale)
    hard = float(al) != 1.0 or defect == "ce_at_alpha1"

    def lse_p(x):
        m = x.max(1).values
        lse = m + torch.log(torch.exp(x - m[:, None]).sum(1))
        return lse, torch.exp(x - lse[:, None])

    lses, qs = lse_p(z * it)
    lset, qt = lse_p(v * it)
    if defect == "kl_swapped":
        kl = (qs * ((z - v) * it)).sum(1)
        kd = (tau * tau) * ((kl - lses) + lset)
        gk = qt - qs          # (not the gradient of anything: the direction is what the case looks at)
    else:
        kl = (qt * ((v - z) * it)).sum(1)
        kd = ((kl - lset) + lses) if defect == "no_tau2" else (tau * tau) * ((kl - lset) + lses)
        gk = qs - qt
    g = (al if defect == "no_tau_dz" else al * tau) * gk
    loss = al * kd
    if hard:
        keep = 1 - t32(eps)
        wa, wb, us = keep * t32(lam), keep * (1 - t32(lam)), t32(eps) / C
        okf = ok.to(F32)
        ac, bc = a.clamp(0, C - 1), b.clamp(0, C - 1)
        lse, p = lse_p(z * it if defect == "temp_on_hard" else z)
        t = (torch.zeros_like(z).scatter_(1, ac[:, None], 1.0) * wa
             + torch.zeros_like(z).scatter_(1, bc[:, None], 1.0) * wb + us) * okf[:, None]
        g = (1 - al) * (p - t) + g
        za, zb = z.gather(1, ac[:, None])[:, 0], z.gather(1, bc[:, None])[:, 0]
        ce = lse - ((wa * za + wb * zb) + us * z.sum(1))
        loss = (1 - al) * ce + loss
        loss = torch.where(ok, loss, torch.full_like(loss, float("nan")))
    h = v if defect == "hits_teacher" else z
    above = (h > h.gather(1, a.clamp(0, C - 1)[:, None])).sum(1)
    rowstat = torch.stack([loss, (ok & (above < 1)).to(F32), (ok & (above < 5)).to(F32)], 1)
    return rowstat, g * gs


CASES = {
    # name: (B, K, C, lam, eps, teacher, temp, alpha, labels) — each defect of DEFECTS fails the case of its
    # name; the others walk the teacher kinds at τ < 1 and τ >= 1
    "no_tau2": (5, 64, 5, 1.0, 0.0, "random", 4.0, 0.5, "planted"),
    "no_tau_dz": (5, 64, 65, 0.3, 0.1, "random", 4.0, 1.0, "planted"),
    "kl_swapped": (5, 64, 5, 1.0, 0.0, "peaky", 0.5, 1.0, "planted"),
    "ce_at_alpha1": (5, 64, 5, 1.0, 0.0, "random", 1.0, 1.0, "unlabelled"),
    "temp_on_hard": (5, 64, 65, 0.3, 0.1, "perm", 4.0, 0.5, "planted"),
    "hits_teacher": (37, 64, 5, 1.0, 0.0, "perm", 1.0, 0.5, "argmax"),
    "equal_cold": (4, 64, 3, 0.5, 0.0, "equal", 0.5, 0.5, "planted"),
    "equal_alpha1": (4, 64, 65, 1.0, 0.0, "equal", 4.0, 1.0, "planted"),
    "perm_cold": (5, 64, 65, 1.0, 0.1, "perm", 0.5, 1.0, "planted"),
    "peaky_hot": (5, 64, 65, 0.3, 0.0, "peaky", 4.0, 0.5, "planted"),
    "const": (5, 64, 5, 1.0, 0.0, "const", 1.0, 0.5, "planted"),
    "const_cold": (5, 64, 1000, 1.0, 0.1, "const", 0.5, 1.0, "planted"),
    "one_class": (4, 64, 1, 1.0, 0.0, "random", 0.5, 0.5, "planted"),
}


def case_inputs(name):
    B, K, C, lam, eps, kind, temp, alpha, labels = CASES[name]
    x, W, b, la, lb = MC.ce_inputs(B, K, C)
    z = (x @ W.t() + b).to(F32)
    if labels == "unlabelled":
        la, lb = torch.full_like(la, -1), torch.full_like(lb, -1)
        la[0] = lb[0] = int(z[0].argmax())        # one labelled row among them: it still scores its hit
    elif labels == "argmax":
        la = z.argmax(1)                           # the student hits every row; a permuted teacher does not
        lb = la.clone()
    else:
        la, lb = MC.plant_labels(z, la, lb, invalid=alpha != 1.0 or B >= 5)
    return z, teacher_rows(z, kind), la, lb, lam, eps, temp, alpha, 1.0 / B


def run_case(impl, name, worst=None):
    """impl(z, v, a, b, lam, eps, temp, alpha, gscale) -> (rowstat, dz) on given logits."""
    z, v, la, lb, lam, eps, temp, alpha, gscale = case_inputs(name)
    rs, dz = impl(z, v, la, lb, lam, eps, temp, alpha, gscale)
    check_distill(worst or MC.Worst(), name, z, v, la, lb, lam, eps, temp, alpha, DO.f32(gscale), rs, dz)
