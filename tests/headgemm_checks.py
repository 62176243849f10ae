"""Bounds, cases, a numpy/torch twin and the checks of the MFMA classifier head
(csrc/kernels/head_gemm.hip) against ``headgemm_oracle``. The same checks run on the twin (CPU,
tests/test_headgemm_oracle.py, where every named defect injected into the twin must be caught)
and on the kernels (tests/test_gpu_headgemm.py).

u = 2^-24 (fp32 unit roundoff). Every bound is derived here, none is measured.

GEMM, kernel against ``split_model`` (bound 1)
    The 3·K' products of bf16 values are exact in fp32 (8 x 8 significant bits), K' the reduction
    length padded to the 64-wide chunk; the padding contributes exact zeros. They are added by
    n_chain = 3·K'/32 chained v_mfma_f32_16x16x32_bf16, the accumulator being one more operand of
    each. The order inside one MFMA is not documented, so every operand of an MFMA, the incoming
    accumulator included, is charged its 32 additions: the hi·hi product of reduction index d
    enters at chain position 3·(d // 32) + 1 and sees W_d = 32·(n_chain − 3·(d // 32)) roundings;
    hi·lo and lo·hi are at most 2^-8 of it and see fewer; |hi| <= (1 + 2^-9)|x|:
        B1 = u·(1 + 2^-7)·Σ_d W_d·|a_d||b_d|                                (γ-style, on Σ|terms|)
    The logits add the bias in fp32 (u·|z|, doubled for the model's own rounding to compare).
GEMM, ``split_model`` against ``exact`` (bound 2)
    x = hi + lo + r with |lo| <= 2^-9|x|, |r| <= 2^-18|x|. The three-term product drops lo·lo and
    the two remainders: |a·b − (ah·bh + ah·bl + al·bh)| = |al·bl + ra·b + a·rb − ra·rb − …|
        B2 = Σ_d (|al||bl| + |ra||b| + |a||rb|)·SECOND_ORDER      (<= 3·2^-18·(1 + 2^-7)·Σ|a||b| = ε₃·Σ|a||b|)
    evaluated from the actual splits, as supcon_oracle.split_bound.
Softmax stage, against an fp64 softmax of the kernel's OWN logits z (fp32 values, exact in fp64)
    m = max z is exact. __expf(x) = exp(x)(1 + δ), |δ| <= K_EXP·(1 + |x|)·u and __logf(l) = log l + ε,
    |ε| <= K_LOG·(1 + |log l|)·u, K_EXP = K_LOG = 4: the model of supcon_checks (the argument times
    log2(e) in fp32, the hardware exp2 / log2 good to about an ulp). The argument x_c = z_c − m is one
    fp32 subtraction: u·|x_c| more. The terms are positive and go through n_add = ceil(C/64) + 6
    additions (lane-strided loop, 6 butterfly steps), so the relative error of l = Σ exp x_c is
        B_l   = u·(Σ_c p_c·(K_EXP·(1 + |x_c|) + |x_c|) + n_add)
        B_lse = B_l·SECOND_ORDER + K_LOG·u·(1 + |log l|) + u·|lse|                (m + log l: one addition)
        B_row = B_lse + u·|lse − z_label|                                          (row loss)
    dz_c = (__expf(z_c − lse) − onehot)·gscale, a_c = z_c − lse (fp32: u·|a_c|, and B_lse from lse):
        Δp_c  = p_c·(B_lse + u·|a_c| + K_EXP·(1 + |a_c|)·u)·SECOND_ORDER
        B_dz  = gscale·(Δp_c + u·|p_c − onehot|) + 2u·|dz_c|                       (gscale = (float)(1/B), the product)
    hit@1 / hit@5 follow the rank rule exactly. NaN loss and zero hits for a label out of range.
Statistics
    stats[j] = (float) Σ_rows rowstat[j] summed in fp64 in row order: where an implementation
    returns its rowstat this is checked EXACTLY (bit for bit) against the fp64 sum of its own rows;
    where it returns only stats: hits exact, |Σ loss| within Σ B_row + u·|Σ|.
Backward GEMMs
    They consume the implementation's own fp32 dz. Where dz is returned (CE head) the model is
    evaluated on it and the bound is B1 alone (+ the epilogue's roundings). Where it is not (probe,
    sweep) the model runs on dz' = fp32(fp64 softmax of the implementation's logits), which differs
    from the implementation's dz by at most e = B_dz + u·|dz|; the three-term product is within ε₃·|a||b| of a·b
    on either side, so
        B_g = B1(dz', x) + Σ_b (e_bc·(1 + 2^-7) + 2ε₃·|dz'_bc|)·|x_bk|
    bias: Σ_b dz in fp32 in row order: B_gb = (B − 1)·u·Σ_b|dz'| + Σ_b e.
SGD  (lr, mom, wd as their fp32 values; the kernel's expressions, contracted or not: every
    operation is charged a rounding of each of its operands' magnitudes)
        d = g + wd·w             B_d   = B_g + 2u·(|g| + |wd·w|)
        buf' = d | mom·buf + d   B_buf = B_d + 2u·(|mom·buf| + |buf'|)          (first: buf ignored)
        w' = w − lr·buf'         B_w   = |lr|·B_buf·SECOND_ORDER + 2u·(|lr·buf'| + |w'|)
CE head sinks
    dW = dW0 + fl(gout·g): B = |gout|·B_g + 2u·|gout·g| + u·|dW|; db alike; dX = fl(gout·acc): |gout|·B1 + 2u·|dX|.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import headgemm_oracle as O
from aux_oracle import f32_value

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
K_EXP = 4.0
K_LOG = 4.0
EPS3 = 3.0 * 2.0 ** -18 * (1.0 + 2.0 ** -7)
SECOND_ORDER = 1.01
TINY = 1e-300

DEFECTS = ("single_bf16", "no_hi_lo", "no_lo_hi", "pad_col", "pad_row", "no_bias", "no_gscale", "no_gout",
           "dw_overwrite", "ignore_first", "lr_index", "wd_index", "logits_layout", "hit_ge", "stats_fp32")


# ------------------------------------------------------------------ bounds ---------------------

def chain_weights(red, red_pad):
    n_chain = 3 * red_pad // 32
    d = torch.arange(red)
    return (32.0 * (n_chain - 3 * (d // 32))).to(F64)


def gemm_bound1(A, Bm, red_pad):
    """A [M][R], Bm [N][R] fp32 -> [M][N]."""
    w = chain_weights(A.shape[1], red_pad)
    return U * (1 + 2.0 ** -7) * ((A.to(F64).abs() * w) @ Bm.to(F64).abs().t())


def gemm_bound2(A, Bm):
    Ah, Al = (t.to(F64) for t in O.split(A))
    Bh, Bl = (t.to(F64) for t in O.split(Bm))
    A, Bm = A.to(F64), Bm.to(F64)
    ra, rb = (A - Ah - Al).abs(), (Bm - Bh - Bl).abs()
    return SECOND_ORDER * (Al.abs() @ Bl.abs().t() + ra @ Bm.abs().t() + A.abs() @ rb.t())


def softmax_bounds(S, gscale):
    """S = O.softmax_stage(z of the implementation) -> dict(row, dz)."""
    z, C = S["z"], S["z"].shape[-1]
    x = (z - S["m"][..., None]).abs()
    n_add = math.ceil(C / 64) + 6
    pl = torch.exp(z - S["m"][..., None]) / S["l"][..., None]
    B_l = U * ((pl * (K_EXP * (1 + x) + x)).sum(-1) + n_add)
    B_lse = B_l * SECOND_ORDER + K_LOG * U * (1 + S["l"].log().abs()) + U * S["lse"].abs()
    row = B_lse + U * (S["lse"] - S["zl"]).abs()
    a = (z - S["lse"][..., None]).abs()
    dp = S["p"] * (B_lse[..., None] + U * a + K_EXP * (1 + a) * U) * SECOND_ORDER
    dz = gscale * (dp + U * (S["p"] - S["onehot"]).abs()) + 2 * U * S["dz"].abs()
    return dict(row=row, dz=dz)


def sgd_ref(w, buf, g, B_g, lr, mom, wd, first):
    """fp64 update and its bounds -> (w', buf', B_w, B_buf)."""
    lr, mom, wd = f32_value(lr), f32_value(mom), f32_value(wd)
    w, buf = w.to(F64), buf.to(F64)
    d = g + wd * w
    B_d = B_g + 2 * U * (g.abs() + (wd * w).abs())
    nb = d if first else mom * buf + d
    B_buf = B_d if first else B_d + 2 * U * ((mom * buf).abs() + nb.abs())
    nw = w - lr * nb
    B_w = abs(lr) * B_buf * SECOND_ORDER + 2 * U * ((lr * nb).abs() + nw.abs())
    return nw, nb, B_w, B_buf


# ------------------------------------------------------------------ cases ----------------------

class Case:
    def __init__(self, name, G, B, K, C, oor, seed):
        self.name, self.G, self.B, self.K, self.C = name, G, B, K, C
        gen = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
        # features with entries spread over 2^±4 around 1, logits of about unit-2 scale
        x = r(B, K) * torch.exp2(8 * torch.rand(B, K, generator=gen, dtype=F64) - 4)
        scale = 2.0 / float(x.pow(2).sum(1).mean().sqrt())
        W = r(G, C, K) * scale
        b = r(G, C) * 0.5
        labels = torch.randint(0, C, (B,), generator=gen)
        labels[0] = C - 1
        if C >= 2:
            # row 0: its label's logit is the row maximum and TIES with class C − 2 in every head
            # (identical weight rows and biases: identical arithmetic), so `>` and `>=` rank apart
            top = 10.0 * x[0] / float(x[0].pow(2).sum())
            W[:, C - 1] = top
            W[:, C - 2] = top
            b[:, C - 2] = b[:, C - 1]
        if oor and B >= 2:
            labels[B - 1] = C if seed % 2 else -1
        self.oor = bool(oor and B >= 2)
        self.x, self.W, self.b, self.labels = x.to(F32), W.to(F32), b.to(F32), labels
        self.bufW = (r(G, C, K) * scale).to(F32)      # garbage the first step must ignore, history of a later one
        self.bufb = (r(G, C) * 0.1).to(F32)
        self.lrs = [0.05 * (g + 1) for g in range(G)]
        self.wds = [1e-3 * (g + 2) for g in range(G)]
        self.mom = 0.9
        self.gout = 1.7
        self.dW0 = (r(C, K) * scale).to(F32)
        self.db0 = (r(C) * 0.1).to(F32)


_SHAPES = [
    # name,            G,  B,  K,    C,    out-of-range label
    ("b1_c1",          1,  1,  64,   1,    0),
    ("b5_c3",          1,  5,  64,   3,    1),
    ("g3_b31_c17",     3,  31, 64,   17,   0),
    ("b33_k192_c63",   1,  33, 192,  63,   1),
    ("b65_c64",        1,  65, 64,   64,   0),
    ("g3_b5_k192_c65", 3,  5,  192,  65,   1),
    ("b31_k2048_c1000", 1, 31, 2048, 1000, 0),
    ("g16_b5_c1030",   16, 5,  64,   1030, 1),
    ("g3_b65_k192_c17", 3, 65, 192,  17,   0),
]
_CASES = {}


def case_names():
    return [s[0] for s in _SHAPES]


def case(name):
    if name not in _CASES:
        i = case_names().index(name)
        _CASES[name] = Case(*_SHAPES[i], seed=100 + i)
    return _CASES[name]


# ------------------------------------------------------------------ the twin -------------------

def _seq_sum32(v):
    """fp32 sum in index order along dim -2."""
    return torch.from_numpy(np.cumsum(v.to(F32).numpy(), axis=-2, dtype=np.float32)[..., -1, :].copy())


class Twin:
    """The kernels' arithmetic in torch on the CPU, tile by tile from the plan mirror: operands
    zero-padded to the tile and to the 64-wide reduction chunk, split into bf16 hi / lo, three
    products per 32 reduction steps, each MFMA one fp32 rounding of (accumulator + 32 exact
    products). ``defect``: one of DEFECTS."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def gemm(self, A, Bm, form, red_is_cols=False, red_is_rows=False):
        """A [M][R], Bm [N][R] -> fp32 [M][N] over the tiles of ``form``."""
        M, R = A.shape
        N = Bm.shape[0]
        assert (M, N, R) == (form["m"], form["n"], form["red"])
        Mp, Np, Rp = form["tiles_m"] * O.TILE, form["tiles_n"] * O.TILE, form["red_pad"]
        tail = 1.0 if ((self.defect == "pad_col" and red_is_cols) or (self.defect == "pad_row" and red_is_rows)) else 0.0
        Ap = torch.zeros(Mp, Rp, dtype=F32)
        Bp = torch.zeros(Np, Rp, dtype=F32)
        Ap[:, R:] = tail
        Bp[:, R:] = tail
        Ap[:M, :R] = A
        Bp[:N, :R] = Bm
        Ah, Al = (t.to(F64) for t in O.split(Ap))
        Bh, Bl = (t.to(F64) for t in O.split(Bp))
        terms = [(Ah, Bh), (Ah, Bl), (Al, Bh)]
        if self.defect == "single_bf16":
            terms = terms[:1]
        elif self.defect == "no_hi_lo":
            terms = [terms[0], terms[2]]
        elif self.defect == "no_lo_hi":
            terms = terms[:2]
        out = torch.zeros(M, N, dtype=F32)
        for bid in range(form["tiles"]):
            tm, tn = divmod(bid, form["tiles_n"])
            m0, n0 = tm * O.TILE, tn * O.TILE
            acc = torch.zeros(O.TILE, O.TILE, dtype=F32)
            for s in range(Rp // 32):
                for P, Q in terms:
                    acc = (acc.to(F64) + P[m0:m0 + O.TILE, 32 * s:32 * s + 32] @ Q[n0:n0 + O.TILE, 32 * s:32 * s + 32].t()).to(F32)
            me, ne = min(m0 + O.TILE, M), min(n0 + O.TILE, N)
            out[m0:me, n0:ne] = acc[:me - m0, :ne - n0]
        return out

    def logits(self, x, W, b, P):
        G, C, K = W.shape
        B = x.shape[0]
        z = self.gemm(x, W.reshape(G * C, K), P["nt"])                      # [B][G·C]
        if self.defect != "no_bias":
            z = (z.to(F64) + b.reshape(1, G * C).to(F64)).to(F32)
        if self.defect == "logits_layout":
            return z.reshape(-1)[:G * B * C].reshape(G, B, C).clone()       # [B][G·C] memory read as [G][B][C]
        return z.reshape(B, G, C).permute(1, 0, 2).contiguous()

    def rows(self, z, labels, B):
        S = O.softmax_stage(z.to(F64), labels, 1.0 if self.defect == "no_gscale" else 1.0 / B)
        rowstat = S["rowstat"].clone()
        if self.defect == "hit_ge":
            ok = S["valid"].expand(rowstat.shape[:-1])
            rowstat[..., 1] = (ok & (S["above_eq"] < 1)).to(F64)
            rowstat[..., 2] = (ok & (S["above_eq"] < 5)).to(F64)
        return S["dz"].to(F32), rowstat.to(F32)

    def stats(self, rowstat):
        if self.defect == "stats_fp32":
            return _seq_sum32(rowstat)
        return O.seq_sum64(rowstat).to(F32)

    def step(self, x, W, b, labels, bufW, bufb, lrs, mom, wds, first, train):
        G, C, K = W.shape
        B = x.shape[0]
        P = O.plan(G, B, K, C)
        z = self.logits(x, W, b, P)
        dz, rowstat = self.rows(z, labels, B)
        out = dict(logits=z, stats=self.stats(rowstat), W=W.clone(), b=b.clone(), bufW=bufW.clone(), bufb=bufb.clone())
        if not train:
            return out
        # TN: rows n = g·C + c of dzᵀ, reduction over the batch
        dzt = dz.permute(0, 2, 1).reshape(G * C, B)
        gW = self.gemm(dzt, x.t().contiguous(), P["tn"], red_is_rows=True).reshape(G, C, K)
        gb = _seq_sum32(dz).reshape(G, C)
        m32 = np.float32(mom)
        for g in range(G):
            lr = np.float32(lrs[(g + 1) % G] if self.defect == "lr_index" else lrs[g])
            wd = np.float32(wds[(g + 1) % G] if self.defect == "wd_index" else wds[g])
            for w, bu, gr in ((out["W"][g], out["bufW"][g], gW[g]), (out["b"][g], out["bufb"][g], gb[g])):
                wn, bn, gn = w.numpy(), bu.numpy(), gr.numpy()
                d = (gn + wd * wn).astype(np.float32)
                nb = d if (first and self.defect != "ignore_first") else (m32 * bn + d).astype(np.float32)
                bn[...] = nb
                wn[...] = (wn - lr * nb).astype(np.float32)
        return out

    def ce(self, x, W, b, labels, gout, dW0, db0):
        C, K = W.shape
        B = x.shape[0]
        P = O.plan(1, B, K, C)
        z = self.logits(x, W[None], b[None], P)
        dz, rowstat = self.rows(z, labels, B)
        z, dz, rowstat = z[0], dz[0], rowstat[0]
        stats = self.stats(rowstat)
        s0 = _seq_sum32(rowstat)[0].double() if self.defect == "stats_fp32" else O.seq_sum64(rowstat)[0]
        go = np.float32(1.0 if self.defect == "no_gout" else gout)
        dX = self.gemm(dz, W.t().contiguous(), P["nn"], red_is_cols=True).numpy() * go
        gW = self.gemm(dz.t().contiguous(), x.t().contiguous(), P["tn"], red_is_rows=True).numpy() * go
        gb = _seq_sum32(dz).numpy() * go
        keep = np.float32(0.0 if self.defect == "dw_overwrite" else 1.0)
        return dict(logits=z, dz=dz, rowstat=rowstat, stats=stats, loss=(s0 / B).to(F32),
                    dX=torch.from_numpy(dX.astype(np.float32)),
                    dW=torch.from_numpy((keep * dW0.numpy() + gW).astype(np.float32)),
                    db=torch.from_numpy((keep * db0.numpy() + gb).astype(np.float32)))


# ------------------------------------------------------------------ checks ---------------------

class Worst:
    """Worst error / bound ratio per quantity."""

    def __init__(self):
        self.r = {}

    def add(self, name, ratio):
        self.r[name] = max(self.r.get(name, 0.0), ratio)

    def report(self):
        return "  ".join(f"{k} {v:.3f}" for k, v in sorted(self.r.items()))


def within(worst, name, got, ref, bound, ctx=""):
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64) if torch.is_tensor(bound) else torch.full_like(ref.to(F64), bound)
    assert got.shape == ref.shape, (ctx, name, got.shape, ref.shape)
    nan_g, nan_r = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_g, nan_r), f"{ctx} {name}: NaN pattern differs"
    err = torch.where(nan_r, torch.zeros_like(ref), (got - ref).abs())
    bound = torch.where(nan_r, torch.ones_like(bound), bound)       # (NaN reference: the pattern is the check)
    assert not bool(torch.isnan(bound).any()), f"{ctx} {name}: NaN bound"
    ratio = float((err / (bound + TINY)).max()) if err.numel() else 0.0
    if worst is not None:
        worst.add(name, ratio)
    assert ratio <= 1.0, f"{ctx} {name}: error/bound {ratio:.3g} (max err {float(err.max()):.3g})"


def same_bits(name, got, ref, ctx=""):
    g, r = got.to(F32).contiguous(), ref.to(F32).contiguous()
    assert g.shape == r.shape and torch.equal(g.view(torch.int32), r.view(torch.int32)), f"{ctx} {name}: not bit-identical"


def _check_logits(worst, ctx, x, W, b, logits, vs_exact):
    G, C, K = W.shape
    B = x.shape[0]
    Wf = W.reshape(G * C, K)
    shape = lambda t: t.reshape(B, G, C).permute(1, 0, 2)  # noqa: E731
    zm = shape(O.three(x, Wf)) + b.to(F64)[:, None, :]
    B1 = shape(gemm_bound1(x, Wf, K)) + 2 * U * zm.abs()
    within(worst, "logits", logits, zm, B1, ctx)
    if vs_exact:
        ze = shape(O.dense(x, Wf)) + b.to(F64)[:, None, :]
        B2 = shape(gemm_bound2(x, Wf))
        within(worst, "split_vs_exact", zm, ze, B2, ctx)
        within(worst, "logits_vs_exact", logits, ze, B1 + B2, ctx)


def _check_stats_sum(worst, ctx, stats, S, SB):
    """stats [..., 3] against the rows of the fp64 softmax stage S of the implementation's logits."""
    ref = O.seq_sum64(S["rowstat"])
    assert torch.equal(torch.nan_to_num(stats[..., 1:].to(F64), nan=-1.0), ref[..., 1:]), f"{ctx} hit counts differ"
    within(worst, "stats_loss", stats[..., 0], ref[..., 0], torch.nan_to_num(SB["row"]).sum(-1) + U * ref[..., 0].abs(), ctx)


def check_step(worst, c, inp, out, vs_exact=False):
    """One probe / sweep step. inp: dict(W, b, bufW, bufb [G…], first, train); out: the
    implementation's dict(logits [G][B][C], stats [G][3], W, b, bufW, bufb after the step)."""
    ctx = f"[{c.name} first={inp['first']} train={inp['train']}]"
    x, W, b = c.x, inp["W"], inp["b"]
    G, C, K = W.shape
    B = x.shape[0]
    P = O.plan(G, B, K, C)
    assert P is not None
    _check_logits(worst, ctx, x, W, b, out["logits"], vs_exact)
    S = O.softmax_stage(out["logits"].to(F64), c.labels, 1.0 / B)
    SB = softmax_bounds(S, 1.0 / B)
    _check_stats_sum(worst, ctx, out["stats"], S, SB)
    if not inp["train"]:
        for k in ("W", "b"):
            same_bits(k + " (eval)", out[k], inp[k], ctx)
        return
    dzr = S["dz"].to(F32)
    e = SB["dz"] + U * S["dz"].abs()
    xa = x.to(F64).abs()
    for g in range(G):
        A = dzr[g].t().contiguous()                     # [C][B]
        gm = O.three(A, x.t())
        B_g = gemm_bound1(A, x.t(), P["tn"]["red_pad"]) + (e[g].t() * (1 + 2.0 ** -7) + 2 * EPS3 * A.to(F64).abs()) @ xa
        wn, bn, B_w, B_buf = sgd_ref(W[g], inp["bufW"][g], gm, B_g, c.lrs[g], c.mom, c.wds[g], inp["first"])
        within(worst, "W", out["W"][g], wn, B_w, ctx + f" head {g}")
        within(worst, "bufW", out["bufW"][g], bn, B_buf, ctx + f" head {g}")
        gb = dzr[g].to(F64).sum(0)
        B_gb = (B - 1) * U * dzr[g].to(F64).abs().sum(0) + e[g].sum(0)
        wn, bn, B_w, B_buf = sgd_ref(b[g], inp["bufb"][g], gb, B_gb, c.lrs[g], c.mom, c.wds[g], inp["first"])
        within(worst, "b", out["b"][g], wn, B_w, ctx + f" head {g}")
        within(worst, "bufb", out["bufb"][g], bn, B_buf, ctx + f" head {g}")


def check_ce(worst, c, out, reduced=True, vs_exact=False):
    """CE head forward + backward on head 0 of the case: out = dict(logits, dz, rowstat, stats,
    loss, dX, dW, db), the sinks started from c.dW0 / c.db0, gout = c.gout."""
    ctx = f"[{c.name} ce]"
    x, W, b = c.x, c.W[0], c.b[0]
    C, K = W.shape
    B = x.shape[0]
    P = O.plan(1, B, K, C)
    _check_logits(worst, ctx, x, W[None], b[None], out["logits"][None], vs_exact)
    S = O.softmax_stage(out["logits"].to(F64), c.labels, 1.0 / B)
    SB = softmax_bounds(S, 1.0 / B)
    rs = out["rowstat"].to(F64)
    assert torch.equal(rs[:, 1:], S["rowstat"][:, 1:]), f"{ctx} hits differ from the rank rule"
    within(worst, "row_loss", rs[:, 0], S["rowstat"][:, 0], SB["row"], ctx)
    within(worst, "dz", out["dz"], S["dz"], SB["dz"], ctx)
    if reduced:
        s64 = O.seq_sum64(out["rowstat"])
        same_bits("stats", torch.nan_to_num(out["stats"], nan=-1.0), torch.nan_to_num(s64.to(F32), nan=-1.0), ctx)
        same_bits("loss", torch.nan_to_num(out["loss"].reshape(1), nan=-1.0),
                  torch.nan_to_num((s64[0] / B).to(F32).reshape(1), nan=-1.0), ctx)
    go = f32_value(c.gout)
    dz = out["dz"]
    Wt = W.t().contiguous()
    dXm = go * O.three(dz, Wt)
    within(worst, "dX", out["dX"], dXm, abs(go) * gemm_bound1(dz, Wt, P["nn"]["red_pad"]) + 2 * U * dXm.abs(), ctx)
    A = dz.t().contiguous()
    gm = go * O.three(A, x.t())
    dWm = c.dW0.to(F64) + gm
    within(worst, "dW", out["dW"], dWm,
           abs(go) * gemm_bound1(A, x.t(), P["tn"]["red_pad"]) + 2 * U * gm.abs() + U * dWm.abs(), ctx)
    gb = go * dz.to(F64).sum(0)
    dbm = c.db0.to(F64) + gb
    within(worst, "db", out["db"], dbm,
           abs(go) * (B - 1) * U * dz.to(F64).abs().sum(0) + 2 * U * gb.abs() + U * dbm.abs(), ctx)


def run_steps(impl, c, worst=None, vs_exact=False, n_steps=2, collect=None):
    """The first and a later training step, then an evaluation, each checked."""
    st = dict(W=c.W.clone(), b=c.b.clone(), bufW=c.bufW.clone(), bufb=c.bufb.clone())
    for i in range(n_steps + 1):
        train = i < n_steps
        inp = dict(st, first=i == 0, train=train)
        out = impl.step(c.x, st["W"].clone(), st["b"].clone(), c.labels, st["bufW"].clone(), st["bufb"].clone(),
                        c.lrs, c.mom, c.wds, i == 0, train)
        check_step(worst, c, inp, out, vs_exact)
        if collect is not None:
            collect.append(out)
        st = {k: out[k] for k in ("W", "b", "bufW", "bufb")}


def run_ce(impl, c, worst=None, vs_exact=False):
    out = impl.ce(c.x, c.W[0].contiguous(), c.b[0].contiguous(), c.labels, c.gout, c.dW0.clone(), c.db0.clone())
    check_ce(worst, c, out, True, vs_exact)
    return out
