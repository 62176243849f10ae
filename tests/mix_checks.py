"""Cases, bounds, fp32 twins and comparisons for Mixup / CutMix (csrc/kernels/mix.hip) and the
soft-target cross-entropy (csrc/include/soft_ce.h) against ``mix_oracle``. The same checks run on
the twins (CPU, tests/test_mix_oracle.py, where every named defect must be caught) and on the
kernels (tests/test_gpu_mix.py). u = 2^-24; every bound is derived here, none is measured.

Mixup, wide regime
    The kernel forms p0 = fl(w0·a), p1 = fl(w1·b), s' = fl(p0 + p1) in fp32 (three roundings, no
    fused multiply-add), then rounds s' to bf16 once. |p0 − w0·a| <= u|w0·a|, p1 alike,
    |s' − (p0 + p1)| <= u|p0 + p1| <= u(1 + u)(|w0·a| + |w1·b|), so with s the exact value
        δ = u·(2·(|w0·a| + |w1·b|))·SECOND_ORDER        >= |s' − s|
    and, rounding being monotone, the stored value lies in [bf16(s − δ), bf16(s + δ)].
    In the exact regime (small integers and halves, λ in quarters) every fp32 operation is exact
    and the stored value IS bf16(s).

Soft cross-entropy, against the fp64 softmax of the implementation's OWN logits z (the logits
are the plain ops' bit for bit; their accuracy is the plain tests' subject). The softmax part is
tests/headgemm_checks.py ``softmax_bounds`` (same expressions, same order: B_lse, Δp_c); the soft
target adds, with keep = fl(1 − ε), wa = fl(keep·λ), wb = fl(keep·fl(1 − λ)), us = fl(ε/C) (λ, ε
taken as their fp32 values; relative errors 2u, 3u, u):
    tgt  = fl(fl(wa·z_a + wb·z_b) + fl(us·fl(Σ_c z_c)))
    Σ_c z_c in fp32 through n_add = ceil(C/64) + 6 additions:  |ΔΣ| <= n_add·u·Σ|z_c|·SECOND_ORDER
    B_tgt = 3u|wa·z_a| + 4u|wb·z_b| + u|wa·z_a + wb·z_b|                   (weights, products, their sum;
            + us·|ΔΣ| + 2u|us·Σz|                                          contracted or not)
            + u|tgt|                                                        (the last addition)
    B_row = B_lse + B_tgt + u|loss|                                         (lse − tgt)
    t_c  = fl(fl(ta + tb) + us):  Δt_c = 2u·wa[c = a] + 3u·wb[c = b] + u·us + 2u|t_c|
    B_dz = gscale·(Δp_c + Δt_c + u|p_c − t_c|) + 2u|dz_c|              (+ FTZ, below)
    fp32 underflow: a result below the smallest normal number 2^-126 is flushed to zero (or rounded
    to a denormal), an absolute error of at most FTZ = 2^-126 that no relative bound covers. It is
    charged to every __expf (Δp_c += FTZ; the sum l >= 1 takes C·FTZ) and to the product by gscale
    (B_dz += FTZ). The exact-regime logits (|z| up to a few hundred) reach it; a trained model's do not.
    Hits follow the rank rule on the implementation's logits exactly.
Against fp64 torch on the INPUTS (the fma rule of tests/test_gpu_ce_head.py: 4 x the error of
fp32 torch on the same inputs + one fp32 ulp of the magnitude) the loss and dz allowances are
extended by max_rows B_tgt / B and gscale·max Δt_c: fp32 torch builds t in fp32 as well but in
another order.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import mix_oracle as MO

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
K_EXP = 4.0
K_LOG = 4.0
SECOND_ORDER = 1.01
FTZ = 2.0 ** -126

MIX_DEFECTS = ("partner_next", "box_inclusive", "lam_after_rounding")
DRAW_DEFECTS = ("lam_uncorrected",)
CE_DEFECTS = ("smooth_c_minus_1", "second_label_unsmoothed", "hits_b", "no_gscale")


# ------------------------------------------------------------------ mixing ---------------------

def boxes(S):
    """name -> (y0, y1, x0, x1): empty, whole, one pixel, touching each edge, a one-column strip."""
    h = max(S // 2, 1)
    return {"empty": (0, 0, 0, 0), "empty_mid": (h, h, 0, S), "whole": (0, S, 0, S), "pixel": (S - 1, S, S - 1, S),
            "top": (0, h, 0, S), "bottom": (S - h, S, 0, S), "left": (0, S, 0, h), "right": (0, S, S - h, S),
            "column": (0, S, S // 2, S // 2 + 1)}


def batch(B, S, seed=0, exact=False):
    """[B, S, S, 8] bf16, all 8 channels filled (the copy must move the padding too)."""
    g = torch.Generator().manual_seed(977 * B + 31 * S + seed)
    if exact:
        return (torch.randint(-8, 9, (B, S, S, 8), generator=g).float() * 0.5).to(torch.bfloat16)
    e = torch.randint(-6, 7, (B, S, S, 8), generator=g).float()
    return (torch.randn(B, S, S, 8, generator=g) * torch.exp2(e)).to(torch.bfloat16)


def mixup_delta(x, lam):
    w0, w1 = MO.mixup_weights(lam)
    return U * 2.0 * ((w0 * x.to(F64)).abs() + (w1 * MO.partner(x).to(F64)).abs()) * SECOND_ORDER


def check_cutmix(got, x, box, ctx=""):
    want = MO.cutmix(x, box)
    assert got.dtype == x.dtype and got.shape == x.shape, ctx
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"cutmix {ctx}: not a bit copy"


def check_mixup_exact(got, x, lam, ctx=""):
    want = MO.round_bf16(MO.mixup_exact(x, lam))
    assert torch.equal(got.float(), want.float()), f"mixup exact {ctx}"


def check_mixup_wide(got, x, lam, ctx=""):
    """-> the largest |got − s| / δ over the elements (recorded in docs/PARITY.md)."""
    s, d = MO.mixup_exact(x, lam), mixup_delta(x, lam)
    lo, hi = MO.round_bf16(s - d).to(F64), MO.round_bf16(s + d).to(F64)
    g = got.to(F64)
    assert bool(((g >= lo) & (g <= hi)).all()), f"mixup wide {ctx}: outside [bf16(s - d), bf16(s + d)]"
    # the fp32 value before the store is not visible; the distance of the stored value from s, less
    # the half-ulp the one rounding may add, over δ
    half_ulp = torch.exp2(torch.floor(torch.log2(s.abs().clamp_min(1e-300))) - 8)
    return float((((g - s).abs() - half_ulp).clamp_min(0) / d.clamp_min(1e-300)).max())


def mix_twin(x, mode, lam, box=(0, 0, 0, 0), defect=None):
    """fp32 torch twin of mix_views on [B, H, W, 8] bf16."""
    xr = x.roll(-1 if defect == "partner_next" else 1, 0)
    if mode == "cutmix":
        y0, y1, x0, x1 = box
        if defect == "box_inclusive":
            y1, x1 = y1 + 1, x1 + 1
        out = x.clone()
        out[:, y0:y1, x0:x1] = xr[:, y0:y1, x0:x1]
        return out
    w0, w1 = MO.mixup_weights(lam)
    if defect == "lam_after_rounding":
        return ((w0 * x.float()).to(torch.bfloat16).float() + (w1 * xr.float()).to(torch.bfloat16).float()
                ).to(torch.bfloat16)
    return (w0 * x.float() + w1 * xr.float()).to(torch.bfloat16)


MIX_CASES = {
    # name: (B, S, mode, lam, box name)
    "partner": (5, 7, "cutmix", 1.0, "whole"),
    "box_end": (2, 7, "cutmix", 1.0, "pixel"),
    "box_column": (2, 7, "cutmix", 1.0, "column"),
    "one_rounding": (5, 7, "mixup", 0.3, None),
}


def run_mix_case(impl, name):
    B, S, mode, lam, bname = MIX_CASES[name]
    x = batch(B, S)
    if mode == "cutmix":
        # the box is moved off the last row / column so that an inclusive end shows
        box = {"pixel": (S - 2, S - 1, S - 2, S - 1)}.get(bname, boxes(S)[bname])
        check_cutmix(impl(x, mode, lam, box), x, box, name)
    else:
        check_mixup_wide(impl(x, mode, lam, (0, 0, 0, 0)), x, lam, name)


# ------------------------------------------------------------------ draws ----------------------

def torchvision_box(lam, r_y, r_x, H, W):
    """Transcription of torchvision.transforms.v2.CutMix.make_params' arithmetic."""
    r = 0.5 * math.sqrt(1.0 - lam)
    r_w_half = int(r * W)
    r_h_half = int(r * H)
    x1 = int(max(r_x - r_w_half, 0))
    y1 = int(max(r_y - r_h_half, 0))
    x2 = int(min(r_x + r_w_half, W))
    y2 = int(min(r_y + r_h_half, H))
    return (y1, y2, x1, x2), float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))


def check_box(fn, n=3000, defect=None):
    rng = np.random.default_rng(5)
    for _ in range(n):
        S = int(rng.integers(1, 65))
        lam, cy, cx = float(rng.beta(1.0, 1.0)), int(rng.integers(S)), int(rng.integers(S))
        box, lam2 = fn(lam, cy, cx, S)
        if defect == "lam_uncorrected":
            lam2 = lam
        wb, wl = torchvision_box(lam, cy, cx, S, S)
        assert tuple(box) == wb and lam2 == wl, (S, lam, cy, cx, box, lam2, wb, wl)
        assert (tuple(box), lam2) == MO.box_rule(lam, cy, cx, S)


# ------------------------------------------------------------------ soft cross-entropy ---------

def softmax_stage_bounds(z, S):
    """tests/headgemm_checks.py softmax_bounds' B_lse and Δp on the fp64 softmax S of z."""
    C = z.shape[1]
    x = (z - S["m"][:, None]).abs()
    ell = torch.exp(z - S["m"][:, None]).sum(1)
    n_add = math.ceil(C / 64) + 6
    pl = torch.exp(z - S["m"][:, None]) / ell[:, None]
    B_l = U * ((pl * (K_EXP * (1 + x) + x)).sum(1) + n_add) + C * FTZ
    B_lse = B_l * SECOND_ORDER + K_LOG * U * (1 + ell.log().abs()) + U * S["lse"].abs()
    a = (z - S["lse"][:, None]).abs()
    dp = S["p"] * (B_lse[:, None] + U * a + K_EXP * (1 + a) * U) * SECOND_ORDER + FTZ
    return B_lse, dp, n_add


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def soft_bounds(z, a, b, lam, eps, gscale):
    """z: the implementation's logits (fp32) -> dict(ref = oracle on z, row, dz, tgt, dt) bounds."""
    z = z.to(F64).cpu()
    lam, eps = f32(lam), f32(eps)
    S = MO.soft_ce(z, a, b, lam, eps, gscale)
    C = z.shape[1]
    B_lse, dp, n_add = softmax_stage_bounds(z, S)
    a_, b_ = torch.as_tensor(a).long().cpu().clamp(0, C - 1), torch.as_tensor(b).long().cpu().clamp(0, C - 1)
    wa, wb, us = (1 - eps) * lam, (1 - eps) * (1 - lam), eps / C
    za, zb = z.gather(1, a_[:, None])[:, 0], z.gather(1, b_[:, None])[:, 0]
    sz, saz = z.sum(1), z.abs().sum(1)
    tgt = wa * za + wb * zb + us * sz
    B_tgt = (3 * U * (wa * za).abs() + 4 * U * (wb * zb).abs() + U * (wa * za + wb * zb).abs()
             + us * n_add * U * saz * SECOND_ORDER + 2 * U * (us * sz).abs() + U * tgt.abs())
    row = B_lse + B_tgt + U * S["loss"].abs().nan_to_num(0.0)
    oa = torch.zeros_like(z).scatter_(1, a_[:, None], 1.0)
    ob = torch.zeros_like(z).scatter_(1, b_[:, None], 1.0)
    dt = (2 * U * wa * oa + 3 * U * wb * ob + U * us + 2 * U * S["t"]) * S["ok"][:, None]
    dz = gscale * (dp + dt + U * (S["p"] - S["t"]).abs()) + 2 * U * S["dz"].abs() + FTZ
    return dict(ref=S, row=row, dz=dz, tgt=B_tgt, dt=dt)


class Worst:
    def __init__(self):
        self.ratio, self.where = 0.0, ""

    def see(self, ratio, where):
        if ratio > self.ratio:
            self.ratio, self.where = ratio, where


def check_soft(worst, ctx, z, a, b, lam, eps, gscale, rowstat, dz):
    """rowstat [B, 3], dz [B, C] of an implementation whose logits are z."""
    Bd = soft_bounds(z, a, b, lam, eps, gscale)
    R = Bd["ref"]
    rs, dz = rowstat.to(F64).cpu(), dz.to(F64).cpu()
    ok = R["ok"]
    assert bool(torch.isnan(rs[~ok, 0]).all()) and not bool(torch.isnan(rs[ok, 0]).any()), f"{ctx}: NaN rows"
    assert torch.equal(rs[:, 1], R["hit1"]) and torch.equal(rs[:, 2], R["hit5"]), f"{ctx}: hits"
    el = (rs[ok, 0] - R["loss"][ok]).abs()
    ed = (dz - R["dz"]).abs()
    if el.numel():
        r = float((el / Bd["row"][ok]).max())
        worst.see(r, f"{ctx} loss")
        assert r <= 1.0, f"{ctx}: row loss error / bound {r:.3f}"
    r = float((ed / Bd["dz"]).max())
    worst.see(r, f"{ctx} dz")
    assert r <= 1.0, f"{ctx}: dz error / bound {r:.3f}"


def soft_twin(z, a, b, lam, eps, gscale, defect=None):
    """fp32 torch twin of soft_ce_row on logits z -> (rowstat [B, 3], dz [B, C])."""
    z = z.to(F32).cpu()
    B, C = z.shape
    a, b = torch.as_tensor(a).long().cpu(), torch.as_tensor(b).long().cpu()
    ok = (a >= 0) & (a < C) & (b >= 0) & (b < C)
    lam32, eps32 = torch.tensor(lam, dtype=F32), torch.tensor(eps, dtype=F32)
    keep = 1 - eps32
    wa, wb = keep * lam32, (1 - lam32 if defect == "second_label_unsmoothed" else keep * (1 - lam32))
    us = eps32 / ((C - 1) if defect == "smooth_c_minus_1" and C > 1 else C)
    okf = ok.to(F32)
    ac, bc = a.clamp(0, C - 1), b.clamp(0, C - 1)
    m = z.max(1).values
    lse = m + torch.log(torch.exp(z - m[:, None]).sum(1))
    t = (torch.zeros_like(z).scatter_(1, ac[:, None], 1.0) * wa + torch.zeros_like(z).scatter_(1, bc[:, None], 1.0) * wb
         + us) * okf[:, None]
    dz = torch.exp(z - lse[:, None]) - t
    if defect != "no_gscale":
        dz = dz * torch.tensor(gscale, dtype=F32)
    za, zb = z.gather(1, ac[:, None])[:, 0], z.gather(1, bc[:, None])[:, 0]
    loss = lse - ((wa * za + wb * zb) + us * z.sum(1))
    loss = torch.where(ok, loss, torch.full_like(loss, float("nan")))
    zh = zb if defect == "hits_b" else za
    above = (z > zh[:, None]).sum(1)
    rowstat = torch.stack([loss, (ok & (above < 1)).to(F32), (ok & (above < 5)).to(F32)], 1)
    return rowstat, dz


def ce_inputs(B, K, C, seed=0, exact=False):
    """x, W, b (fp32) and labels a, b: rows with a = b, a label on the row maximum, and (B >= 4)
    a −1 in either slot are planted by :func:`plant_labels` once the logits are known."""
    g = torch.Generator().manual_seed(1000 * K + 10 * C + B + seed)
    if exact:
        x = torch.randint(-2, 3, (B, K), generator=g).float()
        W = torch.randint(-2, 3, (C, K), generator=g).float()
        b = torch.randint(-2, 3, (C,), generator=g).float() * 0.5
    else:
        x = torch.randn(B, K, generator=g).relu()
        W = torch.randn(C, K, generator=g) / K ** 0.5
        b = 0.1 * torch.randn(C, generator=g)
    la = torch.randint(0, C, (B,), generator=g)
    lb = torch.randint(0, C, (B,), generator=g)
    return x, W, b, la, lb


def plant_labels(z, la, lb, invalid=True):
    """Row 0: a = b; row 1: a on the row maximum (ties included, exact regime); the last two rows
    (B >= 4): −1 as a, −1 as b."""
    la, lb = la.clone(), lb.clone()
    B = la.numel()
    lb[0] = la[0]
    if B > 1:
        la[1] = int(z[1].argmax())
    if invalid and B >= 4:
        la[B - 1] = -1
        lb[B - 2] = -1
    return la, lb


CE_CASES = {
    # name: (B, K, C, lam, eps)
    "smooth": (5, 64, 5, 1.0, 0.1),
    "two_labels": (5, 64, 65, 0.3, 0.1),
    "hits": (37, 64, 5, 0.3, 0.0),
    "gscale": (4, 64, 3, 0.5, 0.0),
}


def run_ce_case(impl, name, worst=None):
    """impl(z, a, b, lam, eps, gscale) -> (rowstat, dz) on given logits."""
    B, K, C, lam, eps = CE_CASES[name]
    x, W, b, la, lb = ce_inputs(B, K, C)
    z = (x @ W.t() + b).to(F32)
    la, lb = plant_labels(z, la, lb)
    if name == "hits":
        # rows whose second label outranks the first: hits counted against b would differ
        lb = z.argmax(1)
        la = z.argmin(1)
    rs, dz = impl(z, la, lb, lam, eps, 1.0 / B)
    check_soft(worst or Worst(), name, z, la, lb, lam, eps, 1.0 / B, rs, dz)
