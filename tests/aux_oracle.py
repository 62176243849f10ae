"""fp64 oracles of three small kernel families, each written from its kernel's header comment:

  csrc/kernels/pool.hip       max-pool forward (values and first-max positions), backward
  csrc/kernels/wprep.hip      fp32 master -> the two bf16 weight layouts; unpad_add
  csrc/kernels/linear_ce.hip  classifier logits, cross-entropy, top-k hits, dz; the SGD step

CPU tensors in, CPU float64 (or int64) out; nothing of the extension is imported.

Max-pool, NHWC. Window (p, q) covers the taps (ddy, ddx), 0 <= ddy, ddx < k, at input pixel
(p·stride − pad + ddy, q·stride − pad + ddx); a tap outside the image is padding and counts as
−inf. y is the maximum over the window; the recorded position is ddy·k + ddx of the FIRST
in-image tap, in scan order (ddy outer, ddx inner), that holds the maximum. A window whose
in-image taps are all −inf therefore records its first in-image tap, never a padded one (torch
does the same). The comparison is numeric: −0 == +0, the first of the two wins the position
and y carries its sign. NaN is outside the contract.

The backward scatters dy through the positions: dx[n, h, w, c] = Σ dy[n, p, q, c] over the
windows whose recorded tap is (h, w); an input pixel no window names gets exactly 0.

Weight prep. For a weight w [K][C][R][S] (a Linear [K][C] is R = S = 1):
  fwd   [K][R][S][Cp]   bf16(w[k][c][r][s]) for c < C, +0 for C <= c < Cp
  dgrad [C][R][S][K]    bf16(w[k][c][r][s])
one nearest-even rounding each, done on the integer pattern (conv_oracle.rne_bf16).

Classifier. z = x·Wᵀ + b; row loss = lse(z) − z[label]; hit@k = #{c: z[c] > z[label]} < k (a
tie with the label is no miss); dz = (softmax(z) − onehot(label)) / B. A label outside [0, C)
gives loss NaN, no hits, and dz = softmax(z) / B. stats = the column sums of the row
statistics. SGD (torch.optim.SGD, dampening 0): g = dzᵀ·x (bias: Σ_rows dz), d = g + wd·w,
buf = d on the first step and m·buf + d afterwards, w −= lr·buf.
"""
from __future__ import annotations

import numpy as np
import torch

from conv_oracle import rne_bf16

F32, F64 = torch.float32, torch.float64
NEG_INF = float("-inf")


def out_size(H, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1


# ---------------------------------------------------------------- max-pool --------------------

def _tap(n_out, size, stride, pad, d):
    """Input coordinate of tap d of every window along one axis, and whether it is in the image."""
    at = torch.arange(n_out) * stride - pad + d
    return at.clamp(0, size - 1), (at >= 0) & (at < size)


def maxpool_fwd(x, k, stride, pad):
    """x [N, H, W, C] -> (y float64 [N, P, Q, C], pos int64 [N, P, Q, C])"""
    x = x.to(F64)
    N, H, W, C = x.shape
    P, Q = out_size(H, k, stride, pad), out_size(W, k, stride, pad)
    y = torch.full((N, P, Q, C), NEG_INF, dtype=F64)
    pos = torch.full((N, P, Q, C), -1, dtype=torch.int64)
    for ddy in range(k):
        hh, hv = _tap(P, H, stride, pad, ddy)
        for ddx in range(k):
            ww, wv = _tap(Q, W, stride, pad, ddx)
            v = x[:, hh][:, :, ww]
            inside = (hv[:, None] & wv[None, :])[None, :, :, None]
            take = inside & ((pos < 0) | (v > y))
            y = torch.where(take, v, y)
            pos = torch.where(take, torch.full_like(pos, ddy * k + ddx), pos)
    assert (pos >= 0).all(), "a window without an in-image tap: pad >= k?"
    return y, pos


def maxpool_bwd(pos, dy, H, W, k, stride, pad):
    """-> (dx [N, H, W, C] float64 before the bf16 store, Σ|term|, the number of terms)"""
    dy = dy.to(F64)
    N, P, Q, C = dy.shape
    dx = torch.zeros(N, H, W, C, dtype=F64)
    mag = torch.zeros_like(dx)
    cnt = torch.zeros(N, H, W, C, dtype=torch.int64)
    for ddy in range(k):
        hh, hv = _tap(P, H, stride, pad, ddy)
        for ddx in range(k):
            ww, wv = _tap(Q, W, stride, pad, ddx)
            here = pos == ddy * k + ddx
            # for one tap the windows name distinct pixels: a plain indexed add, window by window
            for p in torch.nonzero(hv).reshape(-1).tolist():
                qs = torch.nonzero(wv).reshape(-1)
                sel = here[:, p][:, qs]
                g = torch.where(sel, dy[:, p][:, qs], torch.zeros((), dtype=F64))
                dx[:, hh[p], ww[qs]] += g
                mag[:, hh[p], ww[qs]] += g.abs()
                cnt[:, hh[p], ww[qs]] += sel.to(torch.int64)
    return dx, mag, cnt


# ---------------------------------------------------------------- weight prep -----------------

def wprep_layouts(w, Cp):
    """w fp32 [K][C][R][S] or [K][C] -> (fwd [K][R][S][Cp], dgrad [C][R][S][K]) as float64 holding
    bf16 values. Element by element from the definition; no permute of the tensor itself."""
    w4 = w.detach().reshape(w.shape[0], w.shape[1], *(w.shape[2:] if w.dim() == 4 else (1, 1)))
    K, C, R, S = w4.shape
    r = rne_bf16(w4.to(F64)).numpy()
    fwd = np.zeros((K, R, S, Cp))
    t = np.zeros((C, R, S, K))
    for c in range(C):
        for rr in range(R):
            for ss in range(S):
                fwd[:, rr, ss, c] = r[:, c, rr, ss]
                t[c, rr, ss, :] = r[:, c, rr, ss]
    return torch.from_numpy(fwd), torch.from_numpy(t)


def unpad_add(src, dst):
    """dst [..., C] + src[..., :C]"""
    return dst.to(F64) + src.to(F64)[..., :dst.shape[-1]]


# ---------------------------------------------------------------- classifier ------------------

def classifier(x, W, b, labels):
    """-> dict(z [B][C], rowstat [B][3] (loss, hit@1, hit@5), dz [B][C], stats [3], valid [B])"""
    x, W, b = x.to(F64), W.to(F64), b.to(F64)
    B, C = x.shape[0], W.shape[0]
    z = x @ W.T + b
    valid = (labels >= 0) & (labels < C)
    lab = labels.clamp(0, C - 1)
    lse = torch.logsumexp(z, 1)
    zl = z.gather(1, lab[:, None])[:, 0]
    above = (z > zl[:, None]).sum(1)
    nan = torch.full((), float("nan"), dtype=F64)
    zero = torch.zeros((), dtype=F64)
    rowstat = torch.stack([torch.where(valid, lse - zl, nan),
                           torch.where(valid & (above < 1), 1.0, zero),
                           torch.where(valid & (above < 5), 1.0, zero)], 1)
    onehot = torch.zeros(B, C, dtype=F64)
    onehot[torch.arange(B)[valid], lab[valid]] = 1.0
    dz = (torch.exp(z - lse[:, None]) - onehot) / B
    return dict(z=z, rowstat=rowstat, dz=dz, stats=rowstat.sum(0), valid=valid)


def f32_value(v):
    """The fp32 value a double hyper-parameter becomes at the launcher."""
    return float(np.float32(v))


def sgd_step(x, dz, W, b, bufW, bufb, lr, mom, wd, first):
    """One step on fp64 copies -> dict(W, b, bufW, bufb) and, for the bounds, dict(gW_abs = Σ|dz·x|,
    gb_abs = Σ|dz|, gW, gb). lr / mom / wd as the kernel sees them (fp32 values)."""
    x, dz, W, b, bufW, bufb = (t.to(F64) for t in (x, dz, W, b, bufW, bufb))
    lr, mom, wd = f32_value(lr), f32_value(mom), f32_value(wd)
    out = {}
    for name, w, buf, g, g_abs in (("W", W, bufW, dz.T @ x, dz.abs().T @ x.abs()),
                                   ("b", b, bufb, dz.sum(0), dz.abs().sum(0))):
        d = g + wd * w
        nb = d if first else mom * buf + d
        out[name] = w - lr * nb
        out["buf" + name] = nb
        out["g" + name] = g
        out["g" + name + "_abs"] = g_abs
    return out
