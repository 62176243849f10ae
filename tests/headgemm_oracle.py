"""fp64 oracle of the MFMA classifier head (csrc/kernels/head_gemm.hip), independent of the
package: plain torch / numpy on the CPU.

  z[g]   = x·W[g]ᵀ + b[g]                                   logits [G][B][C]
  dz[g]  = (softmax(z[g]) − onehot)·gscale                  gscale = 1/B
  row    = (lse − z_label, hit@1, hit@5), hit@k <=> #{c : z_c > z_label} < k; (NaN, 0, 0) for a
           label outside [0, C)
  gW[g]  = dz[g]ᵀ·x      gb[g] = Σ_b dz[g]      dX = gout·dz·W      (CE head: dW += gout·gW, db += gout·gb)
  SGD    = aux_oracle.sgd_step with head g's lr and wd

``exact`` evaluates this densely in fp64. ``split_model`` evaluates the arithmetic the kernels are
specified to do with the roundings the specification names and no other: every fp32 operand x of
a GEMM is hi = bf16_rne(x), lo = bf16_rne(x − hi) and a product is hi·hi + hi·lo + lo·hi (lo·lo
and the remainder dropped); dz is rounded to fp32 and split again for the two backward GEMMs.
Sums, exp and log are fp64. ``plan`` mirrors csrc/include/head_gemm_plan.h.
"""
from __future__ import annotations

import numpy as np
import torch

import aux_oracle
from supcon_oracle import F32, F64, bf16_rne, split  # noqa: F401  (bf16_rne re-exported for the checks)

TILE = 64
CHUNK = 64
MAX_K, MAX_C, MAX_G = 4096, 32768, 16
ROWS_PER_BLOCK, BIAS_PER_BLOCK = 4, 256
LIM = 1 << 31


def supported(G, B, K, C):
    if not (1 <= G <= MAX_G and B >= 1 and 1 <= C <= MAX_C):
        return False
    if K < 64 or K > MAX_K or K % CHUNK:
        return False
    return B < LIM and G * B * C < LIM and B * K < LIM and G * C * K < LIM and G * B * 3 < LIM and B + CHUNK < LIM


def _form(m, n, red):
    tm, tn, ch = -(-m // TILE), -(-n // TILE), -(-red // CHUNK)
    return dict(m=m, n=n, red=red, tiles_m=tm, tiles_n=tn, red_pad=ch * CHUNK, chunks=ch, tiles=tm * tn)


def plan(G, B, K, C):
    """The launch plan of (G, B, K, C), or None outside the supported range."""
    if not supported(G, B, K, C):
        return None
    return dict(nt=_form(B, G * C, K), nn=_form(B, K, C), tn=_form(G * C, K, B), rows=G * B,
                row_blocks=-(-G * B // ROWS_PER_BLOCK), bias_blocks=-(-G * C // BIAS_PER_BLOCK),
                logits_elems=G * B * C, rowstat_elems=G * B * 3)


FORM_FIELDS = ("m", "n", "red", "tiles_m", "tiles_n", "red_pad", "chunks", "tiles")


def plan_row(G, B, K, C):
    """The line head_gemm_plan_check --dump prints for this case, as a list of ints."""
    p = plan(G, B, K, C)
    row = [G, B, K, C, 0 if p is None else 1]
    if p is not None:
        for f in ("nt", "nn", "tn"):
            row += [p[f][k] for k in FORM_FIELDS]
        row += [p["rows"], p["row_blocks"], p["bias_blocks"], p["logits_elems"], p["rowstat_elems"]]
    return row


def three(A, Bm):
    """Σ_r A[i, r]·Bm[j, r] with both operands split: hi·hi + hi·lo + lo·hi, fp64 sums."""
    Ah, Al = (t.to(F64) for t in split(A))
    Bh, Bl = (t.to(F64) for t in split(Bm))
    return Ah @ Bh.t() + Ah @ Bl.t() + Al @ Bh.t()


def dense(A, Bm):
    return A.to(F64) @ Bm.to(F64).t()


def softmax_stage(z, labels, gscale):
    """Everything that follows from fp64 logits z [..., B, C] and labels [B]."""
    z = z.to(F64)
    C = z.shape[-1]
    labels = labels.long()
    valid = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    m = z.max(-1).values
    l = torch.exp(z - m[..., None]).sum(-1)
    lse = m + torch.log(l)
    idx = lab.expand(z.shape[:-1])[..., None]
    zl = z.gather(-1, idx)[..., 0]
    above = (z > zl[..., None]).sum(-1)
    above_eq = (z >= zl[..., None]).sum(-1) - 1          # the `>=` rule, the label itself not counted
    nan = torch.full((), float("nan"), dtype=F64)
    zero = torch.zeros((), dtype=F64)
    one = torch.ones((), dtype=F64)
    rowstat = torch.stack([torch.where(valid, lse - zl, nan), torch.where(valid & (above < 1), one, zero),
                           torch.where(valid & (above < 5), one, zero)], -1)
    onehot = torch.zeros_like(z)
    onehot.scatter_(-1, idx, 1.0)
    onehot = onehot * valid.to(F64)[:, None]
    p = torch.exp(z - lse[..., None])
    return dict(z=z, valid=valid, m=m, l=l, lse=lse, zl=zl, above=above, above_eq=above_eq, p=p, onehot=onehot,
                rowstat=rowstat, dz=(p - onehot) * gscale)


def seq_sum64(v):
    """Σ in fp64 in index order along dim -2 (rows), as the statistics role sums."""
    return torch.from_numpy(np.cumsum(v.to(F64).numpy(), axis=-2)[..., -1, :].copy())


def _evaluate(prod, x, W, b, labels, gout):
    G, C, K = W.shape
    B = x.shape[0]
    z = prod(x, W.reshape(G * C, K)).reshape(B, G, C).permute(1, 0, 2) + b.to(F64)[:, None, :]
    o = softmax_stage(z, labels, 1.0 / B)
    dz32 = o["dz"].to(F32)
    o["dz32"] = dz32
    o["gW"] = torch.stack([prod(dz32[g].t(), x.t()) for g in range(G)])          # [G][C][K]
    o["gb"] = dz32.to(F64).sum(1)
    o["dX"] = gout * prod(dz32[0], W[0].t())                                         # [B][K]
    o["stats"] = seq_sum64(o["rowstat"])
    return o


def exact(x, W, b, labels, gout=1.0):
    """W [G][C][K], b [G][C]. dz32 is dz itself here (no rounding)."""
    G, C, K = W.shape
    B = x.shape[0]
    z = dense(x, W.reshape(G * C, K)).reshape(B, G, C).permute(1, 0, 2) + b.to(F64)[:, None, :]
    o = softmax_stage(z, labels, 1.0 / B)
    o["gW"] = torch.stack([o["dz"][g].t() @ x.to(F64) for g in range(G)])
    o["gb"] = o["dz"].sum(1)
    o["dX"] = gout * (o["dz"][0] @ W[0].to(F64))
    o["stats"] = seq_sum64(o["rowstat"])
    return o


def split_model(x, W, b, labels, gout=1.0):
    return _evaluate(three, x, W, b, labels, gout)


def sgd(x, dz, W, b, bufW, bufb, lrs, mom, wds, first):
    """aux_oracle.sgd_step per head on the given dz [G][B][C] -> dict of stacked fp64 tensors."""
    outs = [aux_oracle.sgd_step(x, dz[g], W[g], b[g], bufW[g], bufb[g], lrs[g], mom, wds[g], first)
            for g in range(W.shape[0])]
    return {k: torch.stack([o[k] for o in outs]) for k in outs[0]}
