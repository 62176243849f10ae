"""fp64 oracle of the BN3 fold kernels (csrc/kernels/bnfold.hip), written from the formulas of
that file's header comment. CPU tensors in, CPU float64 out; nothing of the package is imported.

The fold never materialises dy3 = A·dz + D·y3 + E (per-channel A, D, E; y3 = a2·W3ᵀ with the
bf16 conv3 weights W3 [C][K]) and rewrites the two GEMMs that consumed it:

  da2 = dy3·W3   = dz·Wd + a2·Mx + b      Wd = diag(A)·W3   (stored [K][C], bf16)
                                          Mx = W3ᵀ·diag(D)·W3   ([K][K], bf16, symmetric)
                                          b  = Eᵀ·W3 + the coherent-rounding correction (fp32)
  dW3 = dy3ᵀ·a2  = diag(A)·G + diag(D)·W3·S + E ⊗ Σa2      G = dzᵀ·a2, S = a2ᵀ·a2
  Σ_rows dz·y3   = Σ_k W3[c][k]·G[c][k]                    (fp64 in the kernel, hi + lo fp32)

The correction: Wd and Mx are rounded to bf16 once and applied to every row, so the row sums of
da2 pick up rows·(mean(dz)·(A·W3 − Wd) + mean(a2)·(Mx − bf16(Mx))); b carries exactly that
row-mean part, with mean(dz)[c] = −(E + D·μ)/A (A ≠ 0) and mean(a2) = cs / rows. It is defined
against the weights that were actually stored, so ``prep_bias`` takes them as arguments.

``unfolded`` is the definition the fold must equal: dy3 materialised in fp64.
"""
from __future__ import annotations

import math

import torch

from conv_oracle import rne_bf16

F32, F64 = torch.float32, torch.float64


def f32(t):
    """One fp32 rounding of fp64 values (nearest-even), kept in fp64."""
    return t.to(F64).to(F32).to(F64)


def split_coef(coef, C):
    c = coef.to(F64).reshape(3, C)
    return c[0], c[1], c[2]


# ---------------------------------------------------------------- the unfolded definition -----

def unfolded(A, D, E, dz, a2, W):
    """dy3 = A·dz + D·(a2·Wᵀ) + E; da2 = dy3·W; dW3 = dy3ᵀ·a2; Σ_rows dz·y3. All fp64."""
    A, D, E, dz, a2, W = (t.to(F64) for t in (A, D, E, dz, a2, W))
    y3 = a2 @ W.T
    dy3 = A * dz + D * y3 + E
    return dict(dy3=dy3, da2=dy3 @ W, dW=dy3.T @ a2, dzy=(dz * y3).sum(0))


def folded(A, D, E, dz, a2, W):
    """The same three quantities through the fold's matrices (unrounded, no correction)."""
    A, D, E, dz, a2, W = (t.to(F64) for t in (A, D, E, dz, a2, W))
    Wd = A[:, None] * W                       # [C][K]
    Mx = W.T @ (D[:, None] * W)               # [K][K]
    b = E @ W                                 # [K]
    G, S, cs = dz.T @ a2, a2.T @ a2, a2.sum(0)
    return dict(da2=dz @ Wd + a2 @ Mx + b, dW=A[:, None] * G + D[:, None] * (W @ S) + E[:, None] * cs[None, :],
                dzy=(W * G).sum(1), Wd=Wd, Mx=Mx, b=b, G=G, S=S, cs=cs)


# ---------------------------------------------------------------- bnfold_prep ----------------

def prep_wd(coef, W):
    """Wd[k][c] = bf16(fl32(A[c]·W[c][k])): one fp32 product (exact in fp64 first: 24 + 8
    bits) and one nearest-even rounding to bf16. Bit-exact in any regime."""
    C, K = W.shape
    A, _, _ = split_coef(coef, C)
    return rne_bf16(f32(A[:, None] * W.to(F64))).T.contiguous()


def prep_mx(coef, W):
    """-> (Mx [K][K] unrounded, Σ_c |W[c][l]·D[c]·W[c][k]|)"""
    C, K = W.shape
    _, D, _ = split_coef(coef, C)
    W = W.to(F64)
    return W.T @ (D[:, None] * W), W.abs().T @ (D.abs()[:, None] * W.abs())


def mean_dz(coef, mu, C):
    """mean(dz)[c] = −(E + D·μ)/A where A ≠ 0, else 0 (the kernel skips those channels)."""
    A, D, E = split_coef(coef, C)
    nz = A != 0
    return torch.where(nz, -(E + D * mu.to(F64)) / torch.where(nz, A, torch.ones_like(A)), torch.zeros_like(A))


def prep_bias(coef, W, mu, cs, rows, wd_stored, mx_stored):
    """b[l] = Σ_c E[c]·W[c][l] + Σ_c mean(dz)[c]·(A[c]·W[c][l] − Wd[l][c])            (mu given)
                               + Σ_k (cs[k]/rows)·(Mx[l][k] − mx_stored[l][k])        (cs given, rows > 0)
    against the stored bf16 weights. -> dict(b, terms = Σ|term|, m1, mean_a2, ex_abs = Σ_c |m1·A·W|)"""
    C, K = W.shape
    A, D, E = split_coef(coef, C)
    W = W.to(F64)
    b = E @ W
    terms = E.abs() @ W.abs()
    m1 = torch.zeros(C, dtype=F64)
    ex_abs = torch.zeros(K, dtype=F64)
    if mu is not None:
        m1 = mean_dz(coef, mu, C)
        r = A[:, None] * W - wd_stored.to(F64).T          # [C][K]
        b = b + m1 @ r
        terms = terms + m1.abs() @ r.abs()
        ex_abs = m1.abs() @ (A[:, None] * W).abs()
    mean_a2 = torch.zeros(K, dtype=F64)
    if cs is not None and rows > 0:
        mean_a2 = cs.to(F64) / rows
        mx, _ = prep_mx(coef, W)
        r = mx - mx_stored.to(F64)                        # [l][k]
        b = b + r @ mean_a2
        terms = terms + r.abs() @ mean_a2.abs()
    return dict(b=b, terms=terms, m1=m1, mean_a2=mean_a2, ex_abs=ex_abs)


# ---------------------------------------------------------------- bnfold_colsum --------------

def colsum(x):
    """-> (Σ_rows x, Σ_rows |x|)"""
    x = x.to(F64)
    return x.sum(0), x.abs().sum(0)


def colsum_partial(x, blocks, threads=256):
    """partial[b][k]: block b owns the 16-byte chunks e (8 channels each, chunk e holds channels
    8·(e mod K/8) ..) with (e mod blocks·threads) div threads == b. -> [blocks][K] fp64"""
    rows, K = x.shape
    K8 = K // 8
    v = x.to(F64).reshape(-1, 8)
    e = torch.arange(v.shape[0])
    slot = ((e % (blocks * threads)) // threads) * K8 + e % K8
    out = torch.zeros(blocks * K8, 8, dtype=F64)
    out.index_add_(0, slot, v)
    return out.reshape(blocks, K)


# ---------------------------------------------------------------- bnfold_wgrad ---------------

def _chunked_matmul(W, S, step=1024):
    out = torch.zeros(W.shape[0], S.shape[1], dtype=F64)
    for l0 in range(0, S.shape[0], step):
        out += W[:, l0:l0 + step] @ S[l0:l0 + step].to(F64)
    return out


def wgrad(coef, G, S, cs, W, sink=None):
    """dW3[c][k] = A[c]·G[c][k] + D[c]·Σ_l W[c][l]·S[l][k] + E[c]·Σ_b cs[b][k] (+ sink).
    -> (value, Σ|term|)"""
    C, K = W.shape
    A, D, E = split_coef(coef, C)
    W, G, cs = W.to(F64), G.to(F64), cs.to(F64)
    ws = _chunked_matmul(W, S)
    ws_abs = _chunked_matmul(W.abs(), S.abs())
    v = A[:, None] * G + D[:, None] * ws + E[:, None] * cs.sum(0)[None, :]
    t = (A[:, None] * G).abs() + D.abs()[:, None] * ws_abs + E.abs()[:, None] * cs.abs().sum(0)[None, :]
    if sink is not None:
        v = v + sink.to(F64)
        t = t + sink.to(F64).abs()
    return v, t


# ---------------------------------------------------------------- bnfold_rowdot --------------

def rowdot(G, W):
    """Σ_k W[c][k]·G[c][k]: the products are exact in fp64 (8 + 24 bits) and math.fsum adds them
    without error, so the value is the correctly rounded sum. -> (value [C], Σ|term| [C])"""
    p = (W.to(F64) * G.to(F64))
    v = torch.tensor([math.fsum(row) for row in p.tolist()], dtype=F64)
    return v, p.abs().sum(1)


def hi_lo(v):
    """The fp32 pair of a fp64 value: hi = fl32(v), lo = fl32(v − hi)."""
    hi = f32(v)
    return hi, f32(v.to(F64) - hi)


def ulp32(x):
    """The spacing of fp32 numbers at |x| (normal range); 0 at 0."""
    x = x.to(F64).abs()
    e = torch.floor(torch.log2(torch.where(x > 0, x, torch.ones_like(x))))
    return torch.where(x > 0, torch.pow(torch.tensor(2.0, dtype=F64), e - 23), torch.zeros_like(x))
