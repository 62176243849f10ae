"""fp64 oracle of the BatchNorm operations (csrc/kernels/bn.hip) and an fp32 twin of each.

The oracle is written from the definition of the operations (the module header of bn.hip and
the reference network, networks/resnet_big.py: ``relu(bn(y) [+ bn'(y') | + x])`` with torch
BatchNorm2d semantics), in plain torch float64 on the CPU. It never looks at how the kernels
order their arithmetic. Activations are NHWC, so every tensor here is ``[rows, C]``.

    forward     mean = Σy / n            var = Σy² / n − mean²   (clamped at 0)
                invstd = 1 / sqrt(var + eps)
                scale = γ·invstd         shift = β − mean·γ·invstd
                running ← (1 − m)·running + m·(mean | var·n / (n − 1))
                out = act(y·scale + shift [+ r·scale2 + shift2 | + r])
    backward    dz = dout where the forward output was > 0, else 0
                dy = A·dz + D·y + E      A = γ·invstd
                                         D = −A·invstd²·Σdz·(y − μ) / n
                                         E = −A·Σdz / n − D·μ
                dγ = Σdz·(y − μ)·invstd  dβ = Σdz      (both × grad_scale)

``eps`` and ``momentum`` are float32 parameters of the operations (they travel in float32
argument structs), so the oracle takes their float32 values as the exact inputs.

The **twin** functions (``twin_*``) compute the same operations the way the module comments of
bn.hip and bn_epilogue.h describe them: float32 arithmetic left to right, per-channel epilogues
in float64 with one cast per result, one bf16 round-to-nearest-even at the end. They stand in
for a correct kernel on a machine without a GPU (tests/test_bn_oracle.py) and take switches that
make them deliberately wrong, so that the bounds of tests/bn_checks.py are shown to be both
reachable and sharp.
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32


# ---------------------------------------------------------------- bf16 helpers ----------------

def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """float32 -> the nearest bf16 value (ties to even), returned as float32. Integer
    arithmetic on the bit pattern; bit-equal to ``x.bfloat16().float()`` for finite x."""
    assert x.dtype == F32
    u = x.contiguous().numpy().view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return torch.from_numpy(r.view(np.float32).copy()).reshape(x.shape)


def bf16_bits(x: torch.Tensor) -> np.ndarray:
    """The 16-bit patterns of a bf16 tensor, or of a float32/float64 tensor that holds bf16
    values exactly."""
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)
    u = x.to(F32).contiguous().numpy().view(np.uint32).reshape(-1)
    assert not (u & np.uint32(0xFFFF)).any(), "not a bf16 value"
    return (u >> np.uint32(16)).astype(np.uint16)


def relu_bits(out: torch.Tensor) -> np.ndarray:
    """Packed uint8 ReLU mask: bit i of byte e is set iff element 8e+i is > 0."""
    flat = (out.reshape(-1).to(F64) > 0).numpy()
    assert flat.size % 8 == 0
    return np.packbits(flat, bitorder="little")


def unpack_bits(bits, n: int) -> torch.Tensor:
    b = bits.numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    return torch.from_numpy(np.unpackbits(b.astype(np.uint8), bitorder="little")[:n].astype(bool))


def _d(x):
    return None if x is None else x.to(F64)


# ---------------------------------------------------------------- oracle: forward -------------

def stats(y: torch.Tensor) -> torch.Tensor:
    """[rows, C] (or any [..., C]) -> [2, C] float64: Σy, Σy²."""
    y = y.to(F64).reshape(-1, y.shape[-1])
    return torch.stack([y.sum(0), (y * y).sum(0)])


def finalize(sums, count, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """-> dict(scale, shift, mean, invstd, running_mean, running_var, rm_terms, rv_terms).
    ``*_terms`` are |(1−m)·old| + |m·new|, the magnitudes the running-statistic bound needs."""
    count = float(count)
    eps = float(np.float32(eps))
    m = float(np.float32(momentum))
    s1, s2 = sums[0].to(F64), sums[1].to(F64)
    C = s1.numel()
    g = _d(gamma) if gamma is not None else torch.ones(C, dtype=F64)
    b = _d(beta) if beta is not None else torch.zeros(C, dtype=F64)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    o = dict(scale=g * invstd, shift=b - mean * g * invstd, mean=mean, invstd=invstd,
             shift_terms=b.abs() + (mean * g * invstd).abs())
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        rm, rv = _d(running_mean), _d(running_var)
        o["running_mean"] = (1.0 - m) * rm + m * mean
        o["running_var"] = (1.0 - m) * rv + m * unbiased
        o["rm_terms"] = ((1.0 - m) * rm).abs() + (m * mean).abs()
        o["rv_terms"] = ((1.0 - m) * rv).abs() + (m * unbiased).abs()
    return o


def eval_affine(gamma, beta, running_mean, running_var, eps):
    eps = float(np.float32(eps))
    C = running_mean.numel()
    g = _d(gamma) if gamma is not None else torch.ones(C, dtype=F64)
    b = _d(beta) if beta is not None else torch.zeros(C, dtype=F64)
    invstd = 1.0 / torch.sqrt(_d(running_var) + eps)
    return g * invstd, b - _d(running_mean) * g * invstd


def apply(y, sc, sh, r=None, sc2=None, sh2=None, res_mode=0, relu=True):
    """-> (z, T): the unrounded float64 value and the magnitude sum
    T = |y·sc| + |sh| [+ |r·sc2| + |sh2|  |  + |r|]."""
    y, sc, sh = _d(y), _d(sc), _d(sh)
    z = y * sc + sh
    T = (y * sc).abs() + sh.abs()
    if res_mode == 1:
        z = z + _d(r) * _d(sc2) + _d(sh2)
        T = T + (_d(r) * _d(sc2)).abs() + _d(sh2).abs()
    elif res_mode == 2:
        z = z + _d(r)
        T = T + _d(r).abs()
    if relu:
        z = z.clamp_min(0.0)
    return z, T


# ---------------------------------------------------------------- oracle: backward ------------
# mask_source: None | ("act", out) | ("bits", uint8 [numel/8]) | ("affine", msc, msh)

def mask_of(mask_source, ya):
    """-> (mask, T) : bool [rows, C] (None: no mask) and, for the affine kind, the magnitude
    |ya·msc| + |msh| of the value whose sign decides the mask (else None)."""
    if mask_source is None:
        return None, None
    kind = mask_source[0]
    if kind == "act":
        return _d(mask_source[1]).reshape(ya.shape) > 0, None
    if kind == "bits":
        return unpack_bits(mask_source[1], ya.numel()).reshape(ya.shape), None
    assert kind == "affine"
    msc, msh = _d(mask_source[1]), _d(mask_source[2])
    return _d(ya) * msc + msh > 0, (_d(ya) * msc).abs() + msh.abs()


def masked(dout, mask):
    """dz: dout where the mask holds, +0 elsewhere (dout itself without a mask)."""
    d = _d(dout)
    return d if mask is None else torch.where(mask, d, torch.zeros((), dtype=F64))


def bwd_sums(dout, mask_source, ya, mu_a, yb=None, mu_b=None):
    """-> (sums, abs_sums, dz): [2|3, C] float64 Σdz, Σdz·(ya−μa) [, Σdz·(yb−μb)], the
    per-channel sums of the absolute terms, and dz."""
    mask, _ = mask_of(mask_source, ya)
    dz = masked(dout, mask)
    terms = [dz, dz * (_d(ya) - _d(mu_a))]
    if yb is not None:
        terms.append(dz * (_d(yb) - _d(mu_b)))
    return torch.stack([t.sum(0) for t in terms]), torch.stack([t.abs().sum(0) for t in terms]), dz


def coef(sums, count, gamma, mu, inv, grad_scale=1.0, set_index=0):
    """-> dict(A, D, E, dgamma, dbeta, E_terms) for BN set ``set_index`` of ``sums``."""
    count = float(count)
    sdz, sdzy = sums[0].to(F64), sums[1 + set_index].to(F64)
    inv, mu = _d(inv), _d(mu)
    g = _d(gamma) if gamma is not None else torch.ones_like(inv)
    A = g * inv
    D = -A * inv * inv * (sdzy / count)
    E = -A * (sdz / count) - D * mu
    return dict(A=A, D=D, E=E, dgamma=sdzy * inv * grad_scale, dbeta=sdz * grad_scale,
                E_terms=(A * (sdz / count)).abs() + (D * mu).abs())


def bwd_apply(dout, mask_source, ya, ca, yb=None, cb=None):
    """ca / cb: [3, C] (A, D, E). -> dict(dya, Ta, dyb, Tb, dz); T = |A·dz| + |D·y| + |E|."""
    mask, _ = mask_of(mask_source, ya)
    dz = masked(dout, mask)
    o = dict(dz=dz, dyb=None, Tb=None)
    for key, y, c in (("a", ya, ca), ("b", yb, cb)):
        if y is None:
            continue
        A, D, E = _d(c[0]), _d(c[1]), _d(c[2])
        o["dy" + key] = A * dz + D * _d(y) + E
        o["T" + key] = (A * dz).abs() + (D * _d(y)).abs() + E.abs()
    return o


# ---------------------------------------------------------------- fp32 twin -------------------
# `wrong`: a set of names, each switching one deliberate defect on (tests/test_bn_oracle.py)

def _f(x):
    return None if x is None else x.to(F32)


def twin_col_reduce(slab: torch.Tensor, wrong=()) -> torch.Tensor:
    """[rows, NS, C] float32 -> [NS, C] float64 sums (float64 accumulation of float32 values)."""
    rows = slab.shape[0]
    if "drop_tail" in wrong:
        rows = rows // 4 * 4
    return slab[:rows].to(F64).sum(0)


def twin_finalize(sums, count, gamma, beta, eps, momentum, running_mean=None, running_var=None, wrong=()):
    count = float(count)
    s1, s2 = sums[0].to(F64), sums[1].to(F64)
    C = s1.numel()
    eps32, m32 = np.float32(eps), torch.tensor(momentum, dtype=F32)
    mean = s1 / (count - 1.0 if "count_minus_one" in wrong else count)
    var = (s2 / count - mean * mean).clamp_min(0.0)
    invstd = (1.0 / torch.sqrt(var + float(eps32))).to(F32)
    g = _f(gamma) if gamma is not None else torch.ones(C, dtype=F32)
    b = _f(beta) if beta is not None else torch.zeros(C, dtype=F32)
    o = dict(scale=g * invstd, shift=b - mean.to(F32) * g * invstd, mean=mean.to(F32), invstd=invstd)
    if running_mean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 and "biased_var" not in wrong else var
        o["running_mean"] = (1.0 - m32) * _f(running_mean) + m32 * mean.to(F32)
        o["running_var"] = (1.0 - m32) * _f(running_var) + m32 * unbiased.to(F32)
    return o


def twin_eval_affine(gamma, beta, running_mean, running_var, eps):
    C = running_mean.numel()
    invstd = torch.rsqrt(_f(running_var) + torch.tensor(eps, dtype=F32))
    g = _f(gamma) if gamma is not None else torch.ones(C, dtype=F32)
    b = _f(beta) if beta is not None else torch.zeros(C, dtype=F32)
    return g * invstd, b - _f(running_mean) * g * invstd


def _wrong_coef(v, wrong):
    """Per-channel vector(s) [..., C] as a defective kernel would index them."""
    if v is None:
        return None
    C = v.shape[-1]
    if "rotate_in_group" in wrong:     # channel i of an 8-channel group reads channel i−1's value
        v = v.reshape(*v.shape[:-1], C // 8, 8).roll(1, -1).reshape(v.shape)
    if "next_group" in wrong:          # channel group e reads group (e+1) % C8
        v = v.reshape(*v.shape[:-1], C // 8, 8).roll(-1, -2).reshape(v.shape)
    return v


def _drop_tail(out: torch.Tensor, wrong) -> torch.Tensor:
    """The last partial block of 256 8-element chunks left unwritten (zero)."""
    if "drop_tail" in wrong:
        flat = out.reshape(-1)
        n8 = flat.numel() // 8
        if n8 % 256:
            flat = flat.clone()
            flat[(n8 // 256) * 256 * 8:] = 0.0
            out = flat.reshape(out.shape)
    return out


def twin_apply(y, sc, sh, r=None, sc2=None, sh2=None, res_mode=0, relu=True, wrong=()):
    """-> bf16 values as float32."""
    if "mode1_as_mode2" in wrong and res_mode == 1:
        res_mode = 2
    sc, sh, sc2, sh2 = (_wrong_coef(_f(v), wrong) for v in (sc, sh, sc2, sh2))
    v = _f(y) * sc + sh
    if res_mode == 1:
        v = v + (_f(r) * sc2 + sh2)
    elif res_mode == 2:
        v = v + _f(r)
    if relu:
        v = v.clamp_min(0.0)
    return _drop_tail(bf16_round(v), wrong)


def _twin_dz(dout, mask_source, ya, wrong=()):
    d = _f(dout)
    if mask_source is None:
        return d
    kind = mask_source[0]
    ge = "mask_ge" in wrong
    if kind == "act":
        o = _f(mask_source[1]).reshape(d.shape)
        mask = o >= 0 if ge else o > 0
    elif kind == "bits":
        mask = unpack_bits(mask_source[1], d.numel()).reshape(d.shape)
    else:
        v = _f(ya) * _wrong_coef(_f(mask_source[1]), wrong) + _wrong_coef(_f(mask_source[2]), wrong)
        mask = v >= 0 if ge else v > 0
    return torch.where(mask, d, torch.zeros((), dtype=F32))


def twin_bwd_sums(dout, mask_source, ya, mu_a, yb=None, mu_b=None, blocks=1, wrong=()):
    """The two-stage reduction of the module comment: every thread of a grid of ``blocks`` x 256
    accumulates its 8-channel chunks (stride blocks·256) in float32, the block folds them in
    float64 into one float32 partial row, and the partial rows are summed in float64."""
    rows, C = dout.shape
    C8 = C // 8
    assert 256 % C8 == 0
    if "mean_b_for_a" in wrong and mu_b is not None:
        mu_a = mu_b
    mu_a = _wrong_coef(_f(mu_a), wrong)
    dz = _twin_dz(dout, mask_source, ya, wrong)
    terms = [dz, dz * (_f(ya) - mu_a)]
    if yb is not None:
        terms.append(dz * (_f(yb) - _wrong_coef(_f(mu_b), wrong)))
    n8, stride = rows * C8, blocks * 256
    n_t = -(-n8 // stride)
    if "drop_tail" in wrong and n8 % stride:
        n_t = max(n_t - 1, 0)
    sums = []
    for t in terms:
        chunks = torch.zeros(max(n_t, 1) * stride, 8, dtype=F32)
        k = min(n8, n_t * stride)
        chunks[:k] = t.reshape(n8, 8)[:k]
        chunks = chunks.reshape(max(n_t, 1), stride, 8)
        acc = torch.zeros(stride, 8, dtype=F32)
        for i in range(chunks.shape[0]):          # sequential float32 accumulation per thread
            acc = acc + chunks[i]
        # thread t of a block owns channel group t % C8; block fold in float64 -> float32 partial
        part = acc.reshape(blocks, 256 // C8, C8, 8).to(F64).sum(1).to(F32)
        sums.append(part.to(F64).sum(0).reshape(C))
    return torch.stack(sums)


def twin_coef(sums, count, gamma, mu, inv, grad_scale=1.0, set_index=0, sink_g=None, sink_b=None, wrong=()):
    """-> dict(coef [3, C] float32, dgamma, dbeta float32 (sink + new when sinks are given))."""
    c = coef(sums, count, _f(gamma) if gamma is not None else None, _f(mu), _f(inv), grad_scale, set_index)
    dg, db = c["dgamma"].to(F32), c["dbeta"].to(F32)
    if "dbeta_unscaled" in wrong:
        db = sums[0].to(F32)
    if "overwrite_sinks" not in wrong:
        dg = dg + _f(sink_g) if sink_g is not None else dg
        db = db + _f(sink_b) if sink_b is not None else db
    return dict(coef=torch.stack([c["A"], c["D"], c["E"]]).to(F32), dgamma=dg, dbeta=db)


def twin_bwd_apply(dout, mask_source, ya, ca, yb=None, cb=None, wrong=()):
    """-> dict(dya, dyb, dz): bf16 values as float32."""
    dz = _twin_dz(dout, mask_source, ya, wrong)
    o = dict(dz=_drop_tail(dz, wrong), dyb=None)
    for key, y, c in (("a", ya, ca), ("b", yb, cb)):
        if y is None:
            continue
        c = _wrong_coef(_f(c), wrong)
        o["dy" + key] = _drop_tail(bf16_round(c[0] * dz + c[1] * _f(y) + c[2]), wrong)
    return o
