"""Inputs, the exactness guard, case tables, derived bounds and comparison functions of the
encoder-to-loss path tests (the oracle: tests/path_oracle.py).

The comparison functions take an *implementation*: ``ExtImpl`` runs the HIP kernels of the
extension, ``TwinImpl`` a CPU fp32 twin (torch fp32 GEMMs of the same exact values, then
``rne_bf16``; the pool and norm kernels in the kernels' summation order), optionally with one named
deliberate defect. tests/test_path_oracle.py holds the twin to the comparisons on the CPU, to half
of every bound, and shows that every defect is caught; tests/test_gpu_path_oracle.py holds the
kernels to the same comparisons; ``python path_checks.py --child <cfg>`` is the fresh process that
runs the head above 2048 rows under a pinned tile config (SDX_CONV_CFG is read once per process).

PROJECTION HEAD, bit-equal. Two regimes from a seeded CPU generator (tests/conv_checks.py):
  unit   feat, W, dz in {−1, 0, 1}, half of them zero;
  wide   integers in [−A, A] (A = 4, smaller where a long reduction would pass the guard): |h|
         and |dh| pass 256 resp. 2, so the bf16 stores really round, ties included.
A quarter of feat carries a half; biases and sinks are integers and halves; b1 cancels the
accumulator of a few hidden units exactly, so ``h > 0`` is decided on a tie; dz carries fractions
of 2^-10 beside its integers: bf16 ties (to even, both ways) and fp32 values bf16 cannot hold, so
the cast really rounds and Σ dz differs from Σ bf16(dz). The guard (conv_checks.Guard) proves that
every partial sum of every quantity stays below 2^24 units of its terms' common power of two;
then everything is compared with torch.equal. No head quantity needed a bound.

GLOBAL AVERAGE POOL. gap_bwd is bit-equal always (both roundings are mirrored by the oracle).
gap_fwd is bit-equal in the exact regime (multiples of 2^-3, sums below 2^24 units: the fp32 sum is
the real sum and y its product with fp32(1/HW) rounded once). In the wide regime (random bf16)
the sequential fp32 sum of HW terms makes HW − 1 roundings, each of a partial sum of at most Σ|x|:
|ŝ − S| <= γ(HW − 1)·Σ|x| with γ(n) = n·u / (1 − n·u), u = 2^-24; the product adds one rounding:
  |y − S·inv| <= (γ(HW − 1)·Σ|x| + u·(|S| + γ(HW − 1)·Σ|x|))·inv.

ROW NORMALISATION (one wave per row, PER = 1, 2, 4 elements per lane for D <= 64, 128, 256).
Σx² is PER fused multiply-adds and a 6-step butterfly on positive terms: relative error
e_s = γ(PER + 6). ASSUMPTION about the device library, not a measurement: sqrtf and the fp32
division are each within 1 ulp (relative 2u). Then
  norm   e_n = sqrt(1 + e_s)·(1 + 2u) − 1
  y      e_y = (1 + 2u)·(1 + u) / (1 − e_n) − 1           (reciprocal, one multiply)
both relative (max(n, eps) is 1-Lipschitz in n, so the clamp does not widen them).
rownorm_bwd: with A = |dy| + |y|·Σ|dy·y| (it bounds |dy|, |y·dot| and their difference) and
m = max(norm, eps), the dot product errs by γ(PER + 6)·Σ|dy·y|, the subtraction and the product
with the reciprocal make 2 + 3 roundings of values of at most A, and y and norm as inputs carry
relative errors r_y, r_n (u each when they are the oracle's values rounded to fp32, e_y and e_n
after the kernel's own forward), which move y·(y·dy) / norm by (2·r_y + r_n)·A:
  |dx − dx*| <= (γ(PER + 6 + 5) + 2·r_y + r_n)·A / m      (absolute: it holds where dx cancels).

NORM STATISTICS. Per row, Σx² is at most ⌈D/64⌉·4 + 4 roundings on positive terms (float4 path:
4 fma per 64 columns and lane; scalar path ⌈D/16⌉ <= that; a 4-step butterfly): ŝ = s·(1 + θ),
|θ| <= e_s = γ(⌈D/64⌉·4 + 4). The kernel then works in fp64 and takes BOTH sums from the same ŝ
(featnorm.hip:110-111): n̂ = sqrt(ŝ) = n·(1 + ε), |ε| <= e_r = sqrt(1 + e_s) − 1 + 2^-52, so its
variance and loss_sec are those of the perturbed norms n̂, exactly, up to fp64 roundings
e64 = (N/64 + 40)·2^-53 of sums of magnitude T = Σn² (+ 2·r·Σn + N·r² for loss_sec). Carried
through the definitions (sd, rms over the global rows; b_r the bound of rec):
  mean      (e_r + e64)·mean                                       + u·|mean|
  var       2·sd·e_r·rms + e_r²·G2/n + 4·e64·G2/n                  + u·|var|
  rec       first call b_r = bound(mean); then (1 − m)·b_r' + m·bound(mean) + u·|rec|
  loss_sec  [Σ_local e_r·n·(2·(|n − rec| + b_r) + e_r·n) + 2·|N·rec − Σn|·b_r + N·b_r²
             + 4·e64·(Σn² + 2·|rec|·Σn + N·rec²)] / n_global        + u·|loss_sec|
  loss_l2   (e_s + e64)·loss_l2                                    + u·|loss_l2|
Where all rows have the same norm sd = 0 and the variance bound falls to ~e_r²·n²: a variance or
loss_sec wrong in the 7th digit of n² fails. The momentum is the binding's fp32 value.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

import conv_checks as CK
import path_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
REGIMES = CK.REGIMES
GUARD = CK.Guard()
RATIO = {}            # quantity -> largest observed error / bound (the bounded quantities)
same = CK.same


def gamma(n):
    return n * U / (1.0 - n * U)


def _ratio(name, err, bound, ctx, frac=1.0):
    """err <= frac·bound everywhere (0 <= 0 passes); records the largest ratio."""
    err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
    bad = ~(err <= frac * bound)
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    RATIO[name] = max(RATIO.get(name, 0.0), float(r.max()))
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name} {ctx}: {int(bad.sum())} of {bad.numel()} beyond {frac:g} x the bound; first {i}: "
                             f"error {float(err[i]):.6g}, bound {float(bound[i]):.6g}")


# ================================================================ projection head ==============
# name -> (rows, D, O1, O2 | None, A of the wide regime); the path each is named for is asserted
# through the host-only planner by tests/test_path_oracle.py.
HEAD_CASES = {
    "one row": (1, 64, 64, 8, 4),
    "ragged tile in every dimension": (5, 64, 64, 8, 4),
    "two M-tiles, 8 K-tiles": (77, 512, 512, 64, 4),
    "production width": (64, 2048, 2048, 128, 3),
    "widths no multiple of 64 (runs: no refusal)": (9, 72, 136, 24, 4),
    "linear": (40, 256, 128, None, 4),
    "above 2048 rows: auto tile": (2056, 64, 64, 8, 2),
}
BIG = "above 2048 rows: auto tile"
CHILD_CFGS = [0, 1, 2, 4, 6]           # with the auto choice 3: the fp32-store GEMMs on 0-3, and on
CHILD_MARKER = "PATH-CFG-OK"           # production's 8-wave tiles 4 and 6
SENTINEL = 12345.0
_FRAC = [0.0, 0.0, 0.0, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 3 * 2.0 ** -8, 2.0 ** -10, 2.0 ** -7 + 2.0 ** -10, 2.0 ** -9]

_inputs = {}


def head_inputs(name, regime):
    """All tensors of one head case (float64 holding fp32 / bf16 values exactly), generated once
    per process and never modified."""
    key = (name, regime)
    if key in _inputs:
        return _inputs[key]
    rows, D, O1, O2, amp = HEAD_CASES[name]
    g = CK._gen(rows, D, O1, O2 or 0, REGIMES.index(regime), 11)

    def ints(shape):
        if regime == "unit":
            return CK._ints(shape, "unit", g)
        return torch.randint(-amp, amp + 1, shape, generator=g).to(F64)

    d = dict(name=name, regime=regime, mlp=O2 is not None)
    d["feat"] = ints((rows, D)) + 0.5 * (torch.randint(0, 4, (rows, D), generator=g) == 0).to(F64)
    d["w1"] = ints((O1, D))
    d["b1"] = CK._pick([0.0, 0.5, -0.5, 1.0, -1.0, -3.0, 2.5, 8.0], O1, g)
    if O2 is not None:
        # hidden units 0..3 of row 0: the accumulator is exactly −b1
        d["b1"][:4] = -(d["feat"][0] @ d["w1"][:4].T)
        d["w2"] = ints((O2, O1))
        d["b2"] = CK._pick([0.0, 0.5, -0.5, 1.0, -3.0, 8.0, -8.0, 2.5], O2, g)
    olast = O2 if O2 is not None else O1
    base = ints((rows, olast))
    lim = 1.0 if regime == "unit" else 2.0          # a fraction only beside |integer| >= lim: bf16(dz) stays
    frac = CK._pick(_FRAC, rows * olast, g).reshape(rows, olast)      # on multiples of 2^-7 resp. 2^-6
    d["dz"] = base.sign() * (base.abs() + frac * (base.abs() >= lim))
    # row 0 always holds a tie that goes down, a tie that goes up, a round-up and a round-down
    e = lim * 2.0 ** -8          # half a bf16 ulp at lim
    d["dz"][0, :4] = torch.tensor([lim + e, lim + 3 * e, lim + 1.5 * e, -(lim + e / 4)], dtype=F64)
    for k, shape in (("sw1", (O1, D)), ("sb1", (O1,)), ("sw2", (O2, O1) if O2 else None), ("sb2", (O2,) if O2 else None)):
        if shape is not None:
            d[k] = torch.randint(-16, 17, shape, generator=g).to(F64) / 2
    _inputs[key] = d
    return d


def unit_of(t):
    """The largest power of two (<= 1) that divides every value of t."""
    for k in range(0, 24):
        s = t * 2.0 ** k
        if torch.equal(s, s.round()):
            return 2.0 ** -k
    raise AssertionError("not dyadic")


_refs = {}


def head_ref(name, regime):
    """The oracle's forward and backward of one case and the guard of every quantity, once."""
    key = (name, regime)
    if key in _refs:
        return _refs[key]
    d = head_inputs(name, regime)
    f = O.head_fwd(d["feat"], d["w1"], d["b1"], d.get("w2"), d.get("b2"))
    b = O.head_bwd(d["dz"], f["fb"], f["h"], d["w1"], d.get("w2"))
    A = torch.abs
    fb, dzb = f["fb"], b["dzb"]
    ud = unit_of(dzb)
    GUARD.add("head acc1", A(fb) @ A(d["w1"]).T + A(d["b1"]), 0.5)
    GUARD.add("head Σdz", 2 * A(d["dz"]).sum(0) + 8.0, 2.0 ** -10)
    if d["mlp"]:
        h, dh = f["h"], b["dh"]
        udh = min(unit_of(dh), 0.5)
        GUARD.add("head z", A(h) @ A(d["w2"]).T + A(d["b2"]), 0.5)
        GUARD.add("head dW2", 2 * A(dzb).T @ A(h) + 8.0, ud * 0.5)
        GUARD.add("head dh acc", A(dzb) @ A(d["w2"]), ud)
        GUARD.add("head Σdh", 2 * A(dh).sum(0) + 8.0, udh)
        GUARD.add("head dW1", 2 * A(dh).T @ A(fb) + 8.0, udh * 0.5)
        GUARD.add("head dfeat", A(dh) @ A(d["w1"]), udh)
    else:
        GUARD.add("head dW1", 2 * A(dzb).T @ A(fb) + 8.0, ud * 0.5)
        GUARD.add("head dfeat", A(dzb) @ A(d["w1"]), ud)
    r = dict(f=f, b=b)
    # the sinks after one and after two backward passes
    grads = dict(sw1=b["dw1"], sb1=b["db1"] if d["mlp"] else b["db_last"])
    if d["mlp"]:
        grads.update(sw2=b["dw2"], sb2=b["db_last"])
    r["sinks"] = [{k: d[k] + t * v for k, v in grads.items()} for t in (1, 2)]
    _refs[key] = r
    return r


def head_cfgs(m, name):
    """Tile config of each GEMM of a case, as head_ops.cpp picks them: cfg 3 up to 2048 rows, the
    planner's auto choice above; the masked dgrad on 3 always (a constant of head_ops.cpp:124,
    not observable from outside). -> dict(fwd1, fwd2, dgrad2 (masked), dgrad1 (fp32 store))"""
    rows, D, O1, O2, _ = HEAD_CASES[name]

    def cfg(kind, cin, cout):
        return 3 if rows <= 2048 else CK.plan(m, kind, (rows, 1, 1, cin, cout, 1, 1, 0))["cfg"]

    if O2 is None:
        return dict(fwd1=cfg("fwd", D, O1), dgrad1=cfg("dgrad", D, O1))
    return dict(fwd1=cfg("fwd", D, O1), fwd2=cfg("fwd", O1, O2), dgrad2=3, dgrad1=cfg("dgrad", D, O1))


class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _b(self, t):
        return None if t is None else t.to(BF16).contiguous().to(self.dev)

    def _v(self, t):
        return None if t is None else t.to(F32).contiguous().to(self.dev)

    @staticmethod
    def _c(t):
        return t.cpu().to(F64)

    # -- head
    def head_fwd(self, feat, w1, b1, w2=None, b2=None, feat_bf16=False):
        z, fb, h = self.m.head_fwd(self._b(feat) if feat_bf16 else self._v(feat), self._b(w1), self._v(b1), self._b(w2),
                                   self._v(b2))
        return self._c(z), self._c(fb), (self._c(h) if w2 is not None else None)

    def head_bwd(self, dz, fb, h, w1, w2, sinks, side=False, times=1):
        """The sinks are views inside one fp32 buffer of sentinels. -> (dfeat of the last pass,
        [the sinks after each pass], sentinels intact)."""
        keys = [k for k in ("sw1", "sb1", "sw2", "sb2") if k in sinks]
        gap, off, at = 16, 16, {}
        for k in keys:
            at[k] = off
            off += -(-sinks[k].numel() // gap) * gap + gap
        buf = torch.full((off,), SENTINEL, dtype=F32, device=self.dev)
        view = {k: buf[at[k]:at[k] + sinks[k].numel()].view(sinks[k].shape) for k in keys}
        for k in keys:
            view[k].copy_(sinks[k].to(F32))
        handle = 0
        if side:
            from simclr_pytorch_distributed_amd.ops import streams
            handle = streams.side(self.dev).cuda_stream
        w1t = self._b(w1.T)
        w2t = self._b(w2.T) if w2 is not None else None
        after = []
        for _ in range(times):
            dfeat = self.m.head_bwd(self._v(dz), self._b(fb), self._b(h), w1t, w2t, view["sw1"], view["sb1"],
                                    view.get("sw2"), view.get("sb2"), handle)
            if side:
                from simclr_pytorch_distributed_amd.ops import streams
                streams.join(self.dev)
            after.append({k: self._c(view[k]) for k in keys})
        keep = torch.ones(off, dtype=torch.bool)
        for k in keys:
            keep[at[k]:at[k] + sinks[k].numel()] = False
        return self._c(dfeat), after, bool((buf.cpu()[keep] == SENTINEL).all())

    # -- pool
    def gap_fwd(self, x):
        return self._c(self.m.gap_fwd(self._b(x)))

    def gap_bwd(self, dy, H, W):
        return self._c(self.m.gap_bwd(self._v(dy), H, W))

    # -- norms
    def rownorm_fwd(self, x, eps):
        y, n = self.m.rownorm_fwd(self._v(x), eps)
        return self._c(y), self._c(n)

    def rownorm_bwd(self, dy, y, n, eps):
        return self._c(self.m.rownorm_bwd(self._v(dy), self._v(y), self._v(n), eps))

    def norm_stats(self, x, mode, sums, n_global, momentum, state):
        """state (rec, valid) and sums live in device tensors the kernel updates in place; they
        are read back after the call. -> (out [5], sums, state)"""
        rec = torch.tensor(state[0], dtype=F32, device=self.dev)
        valid = torch.tensor(state[1], dtype=F32, device=self.dev)
        s = torch.tensor(sums, dtype=F64, device=self.dev)
        out = self.m.norm_stats(self._v(x), mode, s, float(n_global), momentum, rec, valid)
        return self._c(out), s.cpu().tolist(), (rec.item(), valid.item())


HEAD_DEFECTS = ["trunc_cast", "bias_after_round", "z_bf16", "dfeat_bf16", "mask_ge", "db1_unmasked", "db1_from_acc",
                "db_last_from_dzb", "sink_overwrite", "wt_untransposed", "drop_last_chunk"]
POOL_DEFECTS = ["gap_last_pixel", "gap_scale_after_bf16", "gap_bwd_trunc"]
NORM_DEFECTS = ["rownorm_plus_eps", "rownorm_clamped_projection", "rownorm_cols_past_D", "stats_ema_first",
                "stats_sec_local_n", "stats_drop_tail"]
DEFECTS = HEAD_DEFECTS + POOL_DEFECTS + NORM_DEFECTS


def _mm(a, b):
    """A fp32 GEMM (exact on guarded inputs, whatever its order)."""
    return (a.to(F32) @ b.to(F32)).to(F64)


def _f32(t):
    return t.to(F32).to(F64)


def _fma(a, b, c):
    """fp32 fused multiply-add on float32 numpy arrays (the fp64 product of two fp32 is exact)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


class TwinImpl:
    """CPU fp32 twin; ``wrong`` names deliberate defects (DEFECTS)."""

    def __init__(self, wrong=()):
        self.wrong = set(wrong)
        assert self.wrong <= set(DEFECTS)
        self.cast = O.trunc_bf16 if "trunc_cast" in self.wrong else O.rne_bf16

    # -- head
    def head_fwd(self, feat, w1, b1, w2=None, b2=None, feat_bf16=False):
        fb = feat if feat_bf16 else self.cast(feat)
        acc = _mm(fb, w1.T)
        if w2 is None:
            z = _f32(acc + b1)
            h = None
        else:
            if "bias_after_round" in self.wrong:
                h = O.rne_bf16(_f32(O.rne_bf16(acc) + b1).clamp_min(0.0))
            else:
                h = O.rne_bf16(_f32(acc + b1).clamp_min(0.0))
            z = _f32(_mm(h, w2.T) + b2)
        if "z_bf16" in self.wrong:
            z = O.rne_bf16(z)
        if "drop_last_chunk" in self.wrong:
            z = z.clone()
            z[:, -4:] = float("nan")
        return z, fb, h

    def head_bwd(self, dz, fb, h, w1, w2, sinks, side=False, times=1):
        dzb = self.cast(dz)

        def wt(w):      # the data gradient's layout [in][out]
            return w.reshape(w.shape[1], w.shape[0]) if "wt_untransposed" in self.wrong else w.T.contiguous()

        def into(cur, k, g):
            cur[k] = _f32(g) if "sink_overwrite" in self.wrong else _f32(cur[k] + _f32(g))

        cur = {k: v.clone() for k, v in sinks.items()}
        after = []
        for _ in range(times):
            dlast = (dzb if "db_last_from_dzb" in self.wrong else dz).sum(0)
            if w2 is None:
                into(cur, "sb1", dlast)
                into(cur, "sw1", _mm(dzb.T, fb))
                dfeat = _mm(dzb, wt(w1).T)
            else:
                into(cur, "sb2", dlast)
                into(cur, "sw2", _mm(dzb.T, h))
                acc = _mm(dzb, wt(w2).T)
                keep = ((h >= 0) if "mask_ge" in self.wrong else (h > 0)).to(F64)
                dh = O.rne_bf16(acc) * keep
                db1 = O.rne_bf16(acc).sum(0) if "db1_unmasked" in self.wrong else \
                    (acc * keep).sum(0) if "db1_from_acc" in self.wrong else dh.sum(0)
                into(cur, "sb1", db1)
                into(cur, "sw1", _mm(dh.T, fb))
                dfeat = _mm(dh, wt(w1).T)
            if "dfeat_bf16" in self.wrong:
                dfeat = O.rne_bf16(dfeat)
            after.append({k: v.clone() for k, v in cur.items()})
        return dfeat, after, True

    # -- pool: the sequential fp32 sum in pixel order
    def gap_fwd(self, x):
        N, H, W, C = x.shape
        v = x.to(F32).reshape(N, H * W, C)
        acc = torch.zeros(N, C, dtype=F32)
        for i in range(H * W - (1 if "gap_last_pixel" in self.wrong else 0)):
            acc = acc + v[:, i]
        if "gap_scale_after_bf16" in self.wrong:
            acc = O.rne_bf16(acc.to(F64)).to(F32)
        return (acc * torch.tensor(O.inv_hw(H * W), dtype=F32)).to(F64)

    def gap_bwd(self, dy, H, W):
        p = (dy.to(F32) * torch.tensor(O.inv_hw(H * W), dtype=F32)).to(F64)
        r = O.trunc_bf16(p) if "gap_bwd_trunc" in self.wrong else O.rne_bf16(p)
        return r[:, None, None, :].expand(dy.shape[0], H, W, dy.shape[1]).contiguous()

    # -- row normalisation: lane l holds columns l + 64k; PER fma, then the xor butterfly
    def _lanes(self, t, D):
        N = t.shape[0]
        per = 1 if D <= 64 else 2 if D <= 128 else 4
        flat = np.concatenate([t.to(F32).numpy().reshape(-1), np.ones(64 * per, dtype=np.float32)])
        col = np.arange(64 * per)
        v = flat[(np.arange(N)[:, None] * D + col[None, :])].copy()
        if "rownorm_cols_past_D" not in self.wrong:
            v[:, D:] = 0.0
        return v.reshape(N, per, 64), per

    @staticmethod
    def _wave_sum(s):
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, idx ^ o]).astype(np.float32)
        return s[:, 0]

    def rownorm_fwd(self, x, eps):
        N, D = x.shape
        v, per = self._lanes(x, D)
        s = np.zeros((N, 64), dtype=np.float32)
        for k in range(per):
            s = _fma(v[:, k], v[:, k], s)
        nrm = np.sqrt(self._wave_sum(s)).astype(np.float32)
        e = np.float32(eps)
        den = (nrm + e) if "rownorm_plus_eps" in self.wrong else np.maximum(nrm, e)
        inv = (np.float32(1.0) / den).astype(np.float32)
        y = (v * inv[:, None, None]).astype(np.float32).reshape(N, -1)[:, :D]
        return torch.from_numpy(y.copy()).to(F64), torch.from_numpy(nrm.copy()).to(F64)

    def rownorm_bwd(self, dy, y, n, eps):
        N, D = dy.shape
        keep, self.wrong = self.wrong, self.wrong - {"rownorm_cols_past_D"}
        g, per = self._lanes(dy, D)
        yy, _ = self._lanes(y, D)
        self.wrong = keep
        s = np.zeros((N, 64), dtype=np.float32)
        for k in range(per):
            s = _fma(g[:, k], yy[:, k], s)
        nrm, e = n.to(F32).numpy(), np.float32(eps)
        dot = self._wave_sum(s)
        if "rownorm_clamped_projection" not in self.wrong:
            dot = np.where(nrm > e, dot, np.float32(0.0)).astype(np.float32)
        inv = (np.float32(1.0) / np.maximum(nrm, e)).astype(np.float32)
        t = _fma(-yy, np.broadcast_to(dot[:, None, None], yy.shape), g)
        dx = (t * inv[:, None, None]).astype(np.float32).reshape(N, -1)[:, :D]
        return torch.from_numpy(dx.copy()).to(F64)

    # -- norm statistics: 16 lanes per row, float4 or scalar loads, a 4-step butterfly, then fp64
    def norm_stats(self, x, mode, sums, n_global, momentum, state):
        N, D = x.shape
        xs = x.to(F32).numpy()
        vec = D % 4 == 0
        Dk = D - D % 4 if "stats_drop_tail" in self.wrong else D
        s = np.zeros((N, 16), dtype=np.float32)
        if vec:
            pad = np.zeros((N, -(-D // 64) * 64), dtype=np.float32)
            pad[:, :D] = xs
            q = pad.reshape(N, -1, 16, 4)
            for t in range(q.shape[1]):
                for j in (3, 2, 1, 0):
                    s = _fma(q[:, t, :, j], q[:, t, :, j], s)
        else:
            pad = np.zeros((N, -(-D // 16) * 16), dtype=np.float32)
            pad[:, :Dk] = xs[:, :Dk]
            q = pad.reshape(N, -1, 16)
            for t in range(q.shape[1]):
                s = _fma(q[:, t], q[:, t], s)
        idx = np.arange(16)
        for o in (8, 4, 2, 1):
            s = (s + s[:, idx ^ o]).astype(np.float32)
        sq = s[:, 0].astype(np.float64)
        s1, s2 = float(np.sqrt(sq).sum()), float(sq.sum())
        if mode == 0:
            return None, [s1, s2], state
        g1, g2 = (s1, s2) if mode == 1 else sums
        mean = g1 / n_global
        var = g2 / n_global - mean * mean
        mom = float(np.float32(momentum))
        first = not state[1] > 0 and "stats_ema_first" not in self.wrong
        r = float(np.float32(mean if first else (1.0 - mom) * state[0] + mom * mean))
        den = float(N) if "stats_sec_local_n" in self.wrong else n_global
        sec = max(s2 - 2.0 * r * s1 + N * r * r, 0.0) / den
        out = torch.tensor([mean, var, r, sec, s2 / n_global], dtype=F64).to(F32).to(F64)
        return out, [g1, g2], (r, 1.0)


# ---------------------------------------------------------------- head comparisons ------------
TILE = (64, 64)


def check_head(impl, name, regime, side=False, times=2):
    """Forward, backward into prefilled sinks inside a sentinel buffer (``times`` passes): every
    output bit for bit."""
    d, r = head_inputs(name, regime), head_ref(name, regime)
    f, b = r["f"], r["b"]
    ctx = f"(head '{name}' {HEAD_CASES[name][:4]} {regime} side {side})"
    z, fb, h = impl.head_fwd(d["feat"], d["w1"], d["b1"], d.get("w2"), d.get("b2"))
    same("fb", fb, f["fb"], ctx)
    if d["mlp"]:
        same("h", h, f["h"], ctx, TILE)
    same("z", z, f["z"], ctx, TILE)
    sinks = {k: d[k] for k in ("sw1", "sb1", "sw2", "sb2") if k in d}
    dfeat, after, intact = impl.head_bwd(d["dz"], f["fb"], f["h"], d["w1"], d.get("w2"), sinks, side, times)
    same("dfeat", dfeat, b["dfeat"], ctx, TILE)
    assert intact, f"sentinels around the sinks overwritten {ctx}"
    for t in range(times):
        for k in sinks:
            same(f"{k} after pass {t + 1}", after[t][k], r["sinks"][t][k], ctx, TILE if k[1] == "w" else None)
    return z, dfeat, after


def check_head_behaviour(impl, name, regime):
    """side = 0 and the side stream, a bf16 feat, and a second run: identical bits."""
    d, r = head_inputs(name, regime), head_ref(name, regime)
    ctx = f"(head '{name}' {regime})"
    z0, df0, a0 = check_head(impl, name, regime, side=False)
    z1, df1, a1 = check_head(impl, name, regime, side=True)
    same("z, second run", z1, z0, ctx)
    same("dfeat, side stream", df1, df0, ctx)
    for k in a0[-1]:
        same(f"{k}, side stream", a1[-1][k], a0[-1][k], ctx)
    zb, fbb, _ = impl.head_fwd(r["f"]["fb"], d["w1"], d["b1"], d.get("w2"), d.get("b2"), feat_bf16=True)
    same("z from a bf16 feat", zb, z0, ctx)
    same("fb from a bf16 feat", fbb, r["f"]["fb"], ctx)


# ================================================================ global average pool ==========
GAP_CASES = [(1, 1, 1, 8), (3, 4, 4, 64), (2, 7, 7, 2048), (5, 3, 5, 24), (4100, 1, 1, 2048)]
GAP_REGIMES = ("exact", "wide")


def _tie_dy(HW, g, n):
    """fp32 values whose product with fp32(1/HW), rounded to fp32, lies exactly halfway between
    two bf16 values (searched among the neighbours of tie·HW; those found are kept)."""
    inv = np.float32(O.inv_hw(HW))
    m = torch.randint(128, 256, (n,), generator=g).numpy().astype(np.float64)
    e = torch.randint(-6, 4, (n,), generator=g).numpy().astype(np.float64)
    tie = ((2 * m + 1) / 512.0 * 2.0 ** e).astype(np.float32)          # 9 significant bits: a bf16 tie
    start = (tie.astype(np.float64) * HW).astype(np.float32)
    out = start.copy()
    found = np.zeros(n, dtype=bool)
    cand = start.copy()
    for step in [0] + [s for k in range(1, 5) for s in (k, -k)]:
        cand = (start.view(np.int32) + step).view(np.float32)
        hit = ((cand * inv).astype(np.float32) == tie) & ~found
        out[hit] = cand[hit]
        found |= hit
    return out[found]


def gap_inputs(case, regime):
    key = ("gap", case, regime)
    if key in _inputs:
        return _inputs[key]
    N, H, W, C = case
    g = CK._gen(*case, GAP_REGIMES.index(regime), 13)
    if regime == "exact":
        x = torch.randint(-128, 129, (N, H, W, C), generator=g).to(F64) / 8
        dy = torch.randint(-64, 65, (N, C), generator=g).to(F64) / 4
    else:
        x = (torch.randn(N, H, W, C, generator=g) * 3).to(BF16).to(F64)
        dy = torch.randn(N, C, generator=g).to(F64)
        t = torch.from_numpy(_tie_dy(H * W, g, min(N * C // 2, 512))).to(F64)
        dy.reshape(-1)[:2 * t.numel():2] = t
    _inputs[key] = dict(x=x, dy=dy)
    return _inputs[key]


def gap_ref(case, regime):
    key = ("gapref", case, regime)
    if key not in _refs:
        d = gap_inputs(case, regime)
        y, sabs = O.gap_fwd(d["x"])
        if regime == "exact":
            GUARD.add("gap Σ|x|", sabs, 0.125)
        _refs[key] = dict(y=y, sabs=sabs, dx=O.gap_bwd(d["dy"], case[1], case[2]))
    return _refs[key]


def check_gap(impl, case, regime, frac=1.0):
    N, H, W, C = case
    d, r = gap_inputs(case, regime), gap_ref(case, regime)
    ctx = f"(gap {case} {regime})"
    y = impl.gap_fwd(d["x"])
    if regime == "exact":
        same("gap y", y, r["y"].to(F32).to(F64), ctx)
    else:
        HW, inv = H * W, O.inv_hw(H * W)
        gm = gamma(HW - 1)
        bound = (gm * r["sabs"] + U * (r["y"].abs() / inv + gm * r["sabs"])) * inv
        _ratio("gap_fwd y", (y - r["y"]).abs(), bound, ctx, frac)
    same("gap dx", impl.gap_bwd(d["dy"], H, W), r["dx"], ctx)


# ================================================================ row normalisation ============
ROWNORM_D = [1, 8, 63, 64, 65, 100, 128, 129, 192, 255, 256]
ROWNORM_N = [1, 4, 5, 333]
EPS = 1e-12
EPS32 = float(np.float32(EPS))
ROW_KINDS = ["zero", "below eps", "exactly eps", "1e15", "dominant", "dy parallel to y", "random", "random"]


def row_kinds(N, D):
    """The kind of each of the first rows: the special rows rotate with D so that N = 1 meets them all."""
    shift = ROWNORM_D.index(D) if D in ROWNORM_D else 0
    return [ROW_KINDS[(r + shift) % len(ROW_KINDS)] for r in range(min(N, len(ROW_KINDS)))]


def rownorm_inputs(N, D):
    key = ("rownorm", N, D)
    if key in _inputs:
        return _inputs[key]
    g = CK._gen(N, D, 17)
    x = torch.randn(N, D, generator=g)
    dy = torch.randn(N, D, generator=g)
    for r, kind in enumerate(row_kinds(N, D)):
        if kind == "zero":
            x[r] = 0.0
        elif kind == "below eps":
            x[r] *= 1e-14
        elif kind == "exactly eps":
            x[r] = 0.0
            x[r, D - 1] = EPS32
        elif kind == "1e15":
            x[r] *= 1e15
        elif kind == "dominant":
            x[r, D // 2] = 1e6
        elif kind == "dy parallel to y":
            dy[r] = (3.0 * x[r].double() / x[r].double().norm().clamp_min(1e-30)).float()
    d = dict(x=x.to(F64), dy=dy.to(F64))
    d["y"], d["n"] = O.rownorm(d["x"], EPS32)
    d["dx"] = O.rownorm_bwd(d["dy"], d["x"], EPS32)
    _inputs[key] = d
    return d


def rownorm_errors(D):
    per = 1 if D <= 64 else 2 if D <= 128 else 4
    e_n = math.sqrt(1.0 + gamma(per + 6)) * (1.0 + 2 * U) - 1.0
    e_y = (1.0 + 2 * U) * (1.0 + U) / (1.0 - e_n) - 1.0
    return per, e_n, e_y


def check_rownorm(impl, N, D, frac=1.0):
    """Forward; backward from the oracle's y and norms (judged alone); backward chained after the
    implementation's own forward."""
    d = rownorm_inputs(N, D)
    per, e_n, e_y = rownorm_errors(D)
    ctx = f"(rownorm N {N} D {D} rows {row_kinds(N, D)})"
    y, n = impl.rownorm_fwd(d["x"], EPS)
    _ratio("rownorm norms", (n - d["n"]).abs(), e_n * d["n"], ctx, frac)
    _ratio("rownorm y", (y - d["y"]).abs(), e_y * d["y"].abs(), ctx, frac)
    m = d["n"].clamp_min(EPS32)[:, None]
    A = d["dy"].abs() + d["y"].abs() * (d["dy"] * d["y"]).abs().sum(1, keepdim=True)
    y32, n32 = d["y"].to(F32).to(F64), d["n"].to(F32).to(F64)
    alone = impl.rownorm_bwd(d["dy"], y32, n32, EPS)
    _ratio("rownorm dx (alone)", (alone - d["dx"]).abs(), (gamma(per + 11) + 3 * U) * A / m, ctx, frac)
    chained = impl.rownorm_bwd(d["dy"], y, n, EPS)
    # the branch of a row at the clamp is the forward's: compare where both took the oracle's
    agree = ((n > EPS32) == (d["n"] > EPS32))[:, None].expand_as(chained)
    assert agree[d["n"] != EPS32].all(), f"a row changed sides of the clamp {ctx}"
    bound = (gamma(per + 11) + 2 * e_y + e_n) * A / m
    _ratio("rownorm dx (chained)", ((chained - d["dx"]).abs() * agree), bound, ctx, frac)


# ================================================================ norm statistics ==============
STATS_N = [1, 63, 65, 257, 300, 4097]
STATS_D = [1, 3, 4, 64, 100, 102, 128, 260, 1000]
MOMENTA = [1.0, 0.9, 0.1]
OUT = ["mean", "var", "rec", "sec", "l2"]


def stats_inputs(N, D, kind, step=0):
    """kind "random": 3·randn rows; "equal": every row a signed permutation of one vector, so the
    row norms are the same real number and the true variance is 0. step scales by a power of two
    (exact), so the equal rows stay equal."""
    key = ("stats", N, D, kind, step)
    if key in _inputs:
        return _inputs[key]
    g = CK._gen(N, D, 19)
    if kind == "equal":
        base = torch.randn(D, generator=g) * 3
        x = torch.stack([base[torch.randperm(D, generator=g)] * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
                         for _ in range(N)])
    else:
        x = torch.randn(N, D, generator=g) * 3
    _inputs[key] = (x * (1.0, 2.0, 0.5)[step]).to(F64)
    return _inputs[key]


class StatsBounds:
    """The bounds of the module docstring for one call; ``b_rec`` chains over the steps."""

    def __init__(self, D):
        self.e_s = gamma(-(-D // 64) * 4 + 4)
        self.e_r = math.sqrt(1.0 + self.e_s) - 1.0 + 2.0 ** -52
        self.b_rec = None

    def of(self, n_local, n_all, n_global, ref, momentum):
        """n_local: this rank's norms, n_all: the global rows' norms -> dict of bounds."""
        e_s, e_r = self.e_s, self.e_r
        e64 = (n_all.numel() / 64 + 40) * 2.0 ** -53
        G2 = (n_all * n_all).sum().item()
        rms, sd = math.sqrt(G2 / n_global), math.sqrt(max(ref["var"], 0.0))
        b_mean = (e_r + e64) * ref["mean"]
        mom = float(np.float32(momentum))
        b_r = b_mean if self.b_rec is None else (1.0 - mom) * self.b_rec + mom * b_mean
        b_r += U * abs(ref["rec"])
        self.b_rec = b_r
        N, r = n_local.numel(), ref["rec"]
        S1, S2 = n_local.sum().item(), (n_local * n_local).sum().item()
        sec = (e_r * n_local * (2 * ((n_local - r).abs() + b_r) + e_r * n_local)).sum().item() + \
            2 * abs(N * r - S1) * b_r + N * b_r * b_r + 4 * e64 * (S2 + 2 * abs(r) * S1 + N * r * r)
        return dict(mean=b_mean + U * abs(ref["mean"]),
                    var=2 * sd * e_r * rms + e_r * e_r * G2 / n_global + 4 * e64 * G2 / n_global + U * abs(ref["var"]),
                    rec=b_r, sec=sec / n_global + U * abs(ref["sec"]), l2=(e_s + e64) * ref["l2"] + U * abs(ref["l2"]))


def _cmp_stats(out, ref, bounds, ctx, frac, only=OUT):
    for i, k in enumerate(OUT):
        if k in only:
            _ratio(f"norm_stats {k}", abs(out[i].item() - ref[k]), bounds[k], ctx + f" {k}", frac)


def check_norm_stats(impl, N, D, kind, momentum, frac=1.0):
    """Three consecutive mode-1 steps on one in-place state; at every step mode 0 + mode 2 from
    the same state meet the same bounds and return the sums mode 1 used."""
    B = StatsBounds(D)
    state, rec = (0.0, 0.0), None
    mom32 = float(np.float32(momentum))
    for step in range(3):
        x = stats_inputs(N, D, kind, step)
        ctx = f"(norm_stats N {N} D {D} {kind} momentum {momentum} step {step})"
        s1, s2, n = O.norm_sums(x)
        ref = O.norm_finalize(n, s1, s2, float(N), mom32, rec)
        bounds = B.of(n, n, float(N), ref, momentum)
        _, sums, st0 = impl.norm_stats(x, 0, [0.0, 0.0], float(N), momentum, state)
        assert st0 == state, f"mode 0 touched the EMA state {ctx}"
        _ratio("norm_stats Σ‖x‖", abs(sums[0] - s1), (B.e_r + 2.0 ** -45) * s1, ctx, frac)
        _ratio("norm_stats Σ‖x‖²", abs(sums[1] - s2), (B.e_s + 2.0 ** -45) * s2, ctx, frac)
        out2, _, st2 = impl.norm_stats(x, 2, sums, float(N), momentum, state)
        out1, _, state = impl.norm_stats(x, 1, [0.0, 0.0], float(N), momentum, state)
        _cmp_stats(out1, ref, bounds, ctx + " mode 1", frac)
        _cmp_stats(out2, ref, bounds, ctx + " mode 2", frac)
        assert state[1] == 1.0 and st2[1] == 1.0, f"valid not set {ctx}"
        assert state[0] == out1[2].item() and st2[0] == out2[2].item(), f"rec is not the returned value {ctx}"
        if kind == "equal" and N > 1:
            assert ref["var"] < 1e-25 * ref["l2"] and bounds["var"] < 1e-9 * ref["l2"], (ctx, ref["var"], bounds["var"])
        rec = ref["rec"]


def check_norm_stats_two_ranks(impl, N, D, kind, frac=1.0):
    """Two ranks of N rows: mode 0 on each half, the sums added on the host, mode 2 on each half
    with n_global = 2N; the loss_sec / loss_l2 contributions add up to the oracle's of all rows."""
    xa, xb = stats_inputs(N, D, kind, 0), stats_inputs(N, D, kind, 1 if kind == "random" else 0).flip(0)
    ctx = f"(norm_stats two ranks N {N} D {D} {kind})"
    full = torch.cat([xa, xb])
    s1, s2, n = O.norm_sums(full)
    ref = O.norm_finalize(n, s1, s2, 2.0 * N, 1.0, None)
    B = StatsBounds(D)
    bounds = B.of(n, n, 2.0 * N, ref, 1.0)
    sums = [impl.norm_stats(x, 0, [0.0, 0.0], 2.0 * N, 1.0, (0.0, 0.0))[1] for x in (xa, xb)]
    tot = [sums[0][0] + sums[1][0], sums[0][1] + sums[1][1]]
    outs = [impl.norm_stats(x, 2, tot, 2.0 * N, 1.0, (0.0, 0.0))[0] for x in (xa, xb)]
    for o in outs:
        _cmp_stats(o, ref, bounds, ctx, frac, only=("mean", "var", "rec"))
    assert torch.equal(outs[0][:3], outs[1][:3]), f"the ranks disagree on the global statistics {ctx}"
    for i, k in ((3, "sec"), (4, "l2")):
        # the two contributions are each rounded to fp32: one more u each
        _ratio(f"norm_stats two-rank {k}", abs(outs[0][i].item() + outs[1][i].item() - ref[k]),
               bounds[k] + U * abs(ref[k]), ctx + f" {k}", frac)


# ================================================================ pinned-config child ==========

def _child(cfg):
    import signal
    signal.alarm(120)       # the child's own limit: SIGALRM ends it
    assert os.environ.get("SDX_CONV_CFG") == str(cfg), "knob not set"
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    c = head_cfgs(m, BIG)
    assert (c["fwd1"], c["fwd2"], c["dgrad2"], c["dgrad1"]) == (cfg, cfg, 3, cfg), c
    assert head_cfgs(m, "one row")["fwd2"] == 3          # up to 2048 rows the knob does not reach the head
    impl = ExtImpl(m, torch.device("cuda:0"))
    for regime in REGIMES:
        check_head(impl, BIG, regime)
    torch.cuda.synchronize()
    print(CHILD_MARKER)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(int(sys.argv[2]))
