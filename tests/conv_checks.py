"""Inputs, the exactness guard, case tables and comparison functions of the conv oracle tests.

The comparison functions take an *implementation*: ``ExtImpl`` runs the HIP kernels of the
extension, ``TwinImpl`` a CPU fp32 twin (torch's fp32 convolutions of the same integers, which
are exact, then ``conv_oracle.rne_bf16``), optionally with a named deliberate defect.
tests/test_conv_oracle.py holds the twin to the comparisons on the CPU and shows that every
defect is caught; tests/test_gpu_conv_oracle.py holds the kernels to the same comparisons;
``python -m conv_checks --child <set>`` is the fresh process of the environment-knob test.

Two input regimes, from a seeded CPU generator:
  unit   x, w, dy in {−1, 0, 1}, half of them zero: every checked quantity is exact, Σy² too.
  wide   integers in [−4, 4]: |y| passes 256 often, so the bf16 store really rounds (ties
         included). y, dx, dW are bit-exact; Σy² may pass 2^24 and then carries a bound.
Scales, shifts, biases, means, addends and sinks are dyadic (integers and halves), and some BN
inputs are exactly 0 so that ``> 0`` is decided on a tie.

The guard (``Guard``): a quantity is claimed bit-exact only if the Σ|a|·|b| analogue of each of
its values — the largest magnitude any partial sum can reach, in any order — stays below 2^24
units, the unit being the common power of two of the terms (1, or 1/2 or 1/4 with halves).
Then every fp32 partial sum is an integer multiple of the unit below 2^24 units: exact.

The one bounded quantity, Σy² of the forward statistics where a column's total passes 2^24:
a tile's column sum is a chain of at most rows_per_tile fp32 additions (fmaf over the wave
tile's rows, a 16-lane row sum, the waves of the tile), each rounding a partial sum that is
at most the tile's Σy², so a tile errs by at most rows_per_tile·2^-24·Σ_tile y²; the m_tiles
slab rows are then summed (in fp64 here, in fp32 by bn_stats_reduce: m_tiles more roundings
of at most the total). Bound: (rows_per_tile + m_tiles)·2^-24·Σy².
"""
from __future__ import annotations

import os
import sys

import torch
import torch.nn.functional as F

import conv_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LIMIT = 2.0 ** 24
U24 = 2.0 ** -24
REGIMES = ("unit", "wide")

# ---------------------------------------------------------------- case tables -----------------
# (N, H, W, C, K, R, stride, pad): the smallest shapes that reach each path; the expectations are
# fields of conv_plan(..., full=True) and tests/test_conv_oracle.py asserts them.
FWD_CASES = {
    "ragged M, 18 K-tiles": (2, 9, 7, 128, 64, 3, 1, 1),
    "3 K-tiles, ragged N": (4, 16, 16, 192, 320, 1, 1, 0),
    "merged classes": (4, 8, 8, 64, 128, 3, 2, 1),
    "strided 1x1": (4, 8, 8, 256, 512, 1, 2, 0),
    "odd stride 2": (2, 9, 7, 64, 64, 3, 2, 1),
    "odd stride 3": (2, 10, 10, 64, 64, 3, 3, 1),
    "Kdim 72": (8, 8, 8, 8, 64, 3, 1, 1),
    "7x7 stem": (2, 32, 32, 8, 64, 7, 2, 3),
    "auto cfg 6 on DEPTH 6": (4, 8, 8, 1024, 256, 1, 1, 0),
    "single-stage DEPTH 3": (8, 8, 8, 256, 64, 1, 1, 0),
}
PINNED_CFGS = [-1, 0, 1, 2, 3, 4, 5, 6]
# tap tiles 11-13: (N, H = W, C, K), pad-1 stride-1 3x3
TAP_CASES = [(3, 32, 64, 64), (2, 32, 64, 96), (3, 16, 128, 128), (5, 8, 256, 256), (3, 4, 512, 512),
             (5, 4, 64, 128), (2, 56, 64, 64)]
TAP_CFG = {(3, 32, 64, 64): (11, 11), (2, 32, 64, 96): (12, 3), (3, 16, 128, 128): (12, 12),
           (5, 8, 256, 256): (12, 12), (3, 4, 512, 512): (13, 13), (5, 4, 64, 128): (13, 13),
           (2, 56, 64, 64): (11, 11)}          # (forward, dgrad) tile config; K = 96 is no whole 64-chunk
EPI_SHAPES = [FWD_CASES["ragged M, 18 K-tiles"], FWD_CASES["3 K-tiles, ragged N"]]
BIAS_SHAPES = [FWD_CASES["7x7 stem"], FWD_CASES["3 K-tiles, ragged N"]]
CAT_CASES = [(2, 8, 256, 64), (2, 8, 512, 128)]          # (N, H = W, K of dy, K2 of a2 = C)
BNSTAT_SHAPES = [FWD_CASES["ragged M, 18 K-tiles"], FWD_CASES["merged classes"]]
MASKS = ["none", "bits", "affine"]

# weight gradient: (shape, cfg, expected family, expected variant or tile config)
WGRAD_GENERIC = [(FWD_CASES["ragged M, 18 K-tiles"], c) for c in (0, 1, 2, 3, -2)] + \
                [(FWD_CASES["7x7 stem"], c) for c in (0, 1, 2, 3, -2)]


def _w3(N, H, C, K, st):
    return (N, H, H, C, K, 3, st, 1)


def _w1(N, H, C, K, st):
    return (N, H, H, C, K, 1, st, 0)


# tap-reuse 3x3 kernels (cfg 9): the smallest N conv_plan accepts for each width
WGRAD_3X3 = [(_w3(1, 32, 64, 64, 1), "plain"), (_w3(1, 16, 64, 128, 1), "plain"), (_w3(1, 8, 128, 64, 1), "plain"),
             (_w3(2, 4, 64, 64, 1), "plain"),
             (_w3(4, 7, 64, 64, 1), "pad"), (_w3(1, 12, 64, 64, 1), "pad"), (_w3(1, 14, 64, 128, 1), "pad"),
             (_w3(1, 28, 64, 64, 1), "pad"), (_w3(1, 56, 64, 64, 1), "pad"),
             (_w3(1, 64, 64, 64, 2), "s2"), (_w3(1, 32, 64, 128, 2), "s2"), (_w3(1, 16, 128, 64, 2), "s2"),
             (_w3(2, 8, 64, 64, 2), "s2"),
             (_w3(4, 14, 64, 64, 2), "s2pad"), (_w3(1, 24, 64, 64, 2), "s2pad"), (_w3(1, 28, 64, 128, 2), "s2pad"),
             (_w3(1, 56, 64, 64, 2), "s2pad")]
# 1x1 kernels (cfg 10): (shape, variant, bn, setter)
WGRAD_1X1 = [(_w1(1, 8, 128, 128, 1), "pipe", 128, None), (_w1(1, 8, 256, 128, 1), "pipe", 256, None),
             (_w1(2, 8, 128, 128, 2), "pipe", 128, None),            # strided, whole rows (Q = 4)
             (_w1(32, 14, 128, 128, 2), "pipe_gen", 128, None), (_w1(2, 24, 128, 128, 2), "pipe_gen", 128, None),
             (_w1(8, 28, 128, 128, 2), "pipe_gen", 128, None),       # Q = 7, 12, 14
             (_w1(1, 8, 256, 256, 1), "big", 256, ("wgrad1x1_big_set", 2)),
             (_w1(1, 8, 64, 128, 1), "pipe", 128, ("wgrad1x1_pairs_set", 1))]
SPLITK_COUNTS = [2, 3, 4, 5, 12, 13, 16, 17, 20, 33]


def out_hw(shape):
    N, H, W, C, K, R, st, pad = shape
    return O.out_size(H, R, st, pad), O.out_size(W, R, st, pad)


# ---------------------------------------------------------------- inputs ----------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))
    return g


def _ints(shape, regime, g):
    if regime == "unit":
        v = torch.randint(0, 2, shape, generator=g) * 2 - 1
        return (v * torch.randint(0, 2, shape, generator=g)).to(F64)
    return torch.randint(-4, 5, shape, generator=g).to(F64)


def _pick(values, n, g):
    return torch.tensor(values, dtype=F64)[torch.randint(0, len(values), (n,), generator=g)]


_inputs = {}


def inputs(shape, regime):
    """All tensors of one case (float64 holding bf16 / fp32 values exactly), generated once per
    process and never modified."""
    key = (tuple(shape), regime)
    if key in _inputs:
        return _inputs[key]
    N, H, W, C, K, R, st, pad = shape
    P, Q = out_hw(shape)
    g = _gen(*shape, REGIMES.index(regime))
    d = dict(shape=shape, regime=regime, P=P, Q=Q)
    d["x"] = _ints((N, H, W, C), regime, g)
    d["w"] = _ints((K, R, R, C), regime, g)
    d["wt"] = d["w"].permute(3, 1, 2, 0).contiguous()
    d["dy"] = _ints((N, P, Q, K), regime, g)
    # operand prologue relu(x·s + t): x·s + t is exactly 0 for many elements (a tie of the ReLU)
    d["in_sc"] = _pick([0.5, 1.0, 1.0, 2.0, -1.0, -0.5], C, g)
    d["in_sh"] = _pick([0.0, 0.0, 0.5, 1.0, -1.0, -0.5, 2.0], C, g)
    d["bias"] = _pick([0.0, 0.5, -0.5, 1.0, -3.0, 8.0, -8.0, 2.5], K, g)
    # epilogue operands of the data gradient, on dx's [N, H, W, C]
    d["addend"] = _ints((N, H, W, C), regime, g)
    d["addend_c"] = _ints((N, -(-H // 2), -(-W // 2), C), regime, g)
    d["abits"] = torch.randint(0, 256, (N * H * W * C // 8,), generator=g).to(torch.uint8)
    d["ya"] = torch.randint(-2, 3, (N, H, W, C), generator=g).to(F64)
    d["yb"] = torch.randint(-2, 3, (N, H, W, C), generator=g).to(F64)
    d["ma"] = _pick([0.0, 0.5, -0.5, 1.0, -1.0], C, g)
    d["mb"] = _pick([0.0, 0.5, -0.5, 1.0, -1.0], C, g)
    d["msc"] = _pick([1.0, -1.0, 0.5, -0.5, 2.0], C, g)
    d["msh"] = _pick([0.0, 0.0, 0.5, -0.5, 1.0, -1.0], C, g)      # ya·msc + msh == 0 happens
    d["bits"] = torch.randint(0, 256, (N * H * W * C // 8,), generator=g).to(torch.uint8)
    d["sink"] = torch.randint(-8, 9, (K, R, R, C), generator=g).to(F64)
    _inputs[key] = d
    return d


def cat_inputs(case, regime):
    N, H, K, K2 = case
    key = ("cat", case, regime)
    if key not in _inputs:
        g = _gen(*case, 7, REGIMES.index(regime))
        C = K2
        _inputs[key] = dict(dy=_ints((N, H, H, K), regime, g), a2=_ints((N, H, H, K2), regime, g),
                            wcat=_ints((C, 1, 1, K + K2), regime, g),
                            bias=_pick([0.0, 0.5, -0.5, 1.0, -3.0, 8.0, 2.5], C, g),
                            ya=torch.randint(-2, 3, (N, H, H, C), generator=g).to(F64),
                            ma=_pick([0.0, 0.5, -0.5, 1.0, -1.0], C, g))
    return _inputs[key]


def mask_of(d, kind):
    return {"none": None, "bits": ("bits", d["bits"]), "affine": ("affine", d["msc"], d["msh"])}[kind]


# ---------------------------------------------------------------- the guard -------------------

class Guard:
    """Collects, per claimed-exact quantity, the largest magnitude a partial sum can reach in
    units of the terms' common power of two; ``ok`` iff all are below 2^24."""

    def __init__(self):
        self.worst = {}

    def add(self, name, bound, unit=1.0):
        v = float(bound.max() if isinstance(bound, torch.Tensor) else bound) / unit
        self.worst[name] = max(self.worst.get(name, 0.0), v)
        assert v < LIMIT, f"exactness guard: {name} can reach {v:.4g} >= 2^24 units: a wrong case, fix its inputs"


GUARD = Guard()


def _abs(t):
    return None if t is None else t.abs()


# ---------------------------------------------------------------- implementations -------------

def plan(m, kind, shape, cfg=-1, in_bn=False, bnstat=False, cat_ch=0, splits=0, accumulate=False):
    N, H, W, C, K, R, st, pad = shape
    return m.conv_plan(N, H, W, C, K, R, R, st, pad, kind == "dgrad", True, kind, in_bn, bnstat, cat_ch, splits, cfg,
                       accumulate)


TILE_M = {0: 128, 1: 256, 2: 64, 3: 64, 4: 128, 5: 256, 6: 128, 11: 256, 12: 256, 13: 128}
TILE_N = {0: 128, 1: 64, 2: 256, 3: 64, 4: 128, 5: 128, 6: 256, 11: 64, 12: 128, 13: 128}


class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _b(self, t):
        return None if t is None else t.to(BF16).contiguous().to(self.dev)

    def _v(self, t):
        return None if t is None else t.to(F32).contiguous().to(self.dev)

    def _u(self, t):
        return None if t is None else t.contiguous().to(self.dev)

    def tiles(self, kind, shape, cfg, **kw):
        """-> (bm, bn, plain): the plan's tile and whether slab row mt holds rows [mt·bm, ...)."""
        p = plan(self.m, kind, shape, cfg, **kw)
        plain = p["tap"][0] == 0 and (kind == "fwd" or shape[6] == 1)
        return TILE_M[p["cfg"]], TILE_N[p["cfg"]], plain

    def fwd(self, x, w, st, pad, cfg=-1, stats=True, sc=None, sh=None, bm=None):
        y, slab = self.m.conv_fwd(self._b(x), self._b(w), st, pad, stats, cfg, self._v(sc), self._v(sh))
        return y.cpu().to(F64), (slab.cpu().to(F64) if stats else None)

    def fwd_bias(self, x, w, st, pad, bias, relu):
        return self.m.conv_fwd_bias(self._b(x), self._b(w), st, pad, self._v(bias), relu).cpu().to(F64)

    def dgrad(self, dy, wt, H, W, st, pad, cfg=-1, addend=None, abits=None, asub=0):
        return self.m.conv_dgrad(self._b(dy), self._b(wt), H, W, st, pad, cfg, None, self._b(addend), self._u(abits),
                                 asub).cpu().to(F64)

    def dgrad_cat(self, dy, wcat, a2, bias, cfg=-1, ya=None, ma=None, bm=None):
        r = self.m.conv_dgrad_cat(self._b(dy), self._b(wcat), self._b(a2), self._v(bias), cfg, self._b(ya), self._v(ma))
        return r[0].cpu().to(F64), (r[1].cpu().to(F64) if ya is not None else None)

    def dgrad_bnstat(self, dy, wt, H, W, st, pad, cfg, ya, ma, yb=None, mb=None, mask=None, addend=None, abits=None,
                     asub=0, store_masked=0, extra_rows=0, bm=None):
        kw = {}
        if mask is not None and mask[0] == "bits":
            kw["mask_bits"] = self._u(mask[1])
        elif mask is not None:
            kw["msc"], kw["msh"] = self._v(mask[1]), self._v(mask[2])
        ya_t = self._b(ya) if ya is not None else torch.empty(0, dtype=BF16, device=self.dev)
        dx, slab = self.m.conv_dgrad_bnstat(self._b(dy), self._b(wt), H, W, st, pad, cfg, None, self._b(addend),
                                            self._u(abits), ya_t, self._v(ma), self._b(yb), self._v(mb),
                                            addend_sub=asub, store_masked=store_masked, extra_rows=extra_rows, **kw)
        return dx.cpu().to(F64), slab.cpu().to(F64)

    def wgrad(self, dy, x, R, st, pad, splits=0, cfg=-1, sink=None, layout="krsc", accumulate=True, sc=None, sh=None):
        out = None
        if sink is not None:
            s = sink.to(F32).to(self.dev)
            out = s.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last) if layout == "cl" else s.contiguous()
        dw = self.m.conv_wgrad(self._b(dy), self._b(x), R, R, st, pad, splits, cfg, out, accumulate and out is not None,
                               self._v(sc), self._v(sh))
        if sink is not None and layout == "cl":
            dw = dw.permute(0, 2, 3, 1)
        return dw.cpu().to(F64).contiguous()


DEFECTS = ["trunc_store", "stats_from_stored", "addend_pre", "split_drop_pixel", "tail_k_channel",
           "pad_tap_neighbour", "dup_split", "sink_overwrite"]


def _nchw(t):
    return t.permute(0, 3, 1, 2).to(F32).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).to(F64).contiguous()


class TwinImpl:
    """CPU fp32 twin: torch fp32 convolutions (exact on these inputs) and ``rne_bf16``.
    ``wrong`` names deliberate defects (DEFECTS)."""

    def __init__(self, wrong=()):
        self.wrong = set(wrong)
        assert self.wrong <= set(DEFECTS)
        self.round = O.trunc_bf16 if "trunc_store" in self.wrong else O.rne_bf16

    def tiles(self, kind, shape, cfg, **kw):
        return 128, 128, kind == "fwd" or shape[6] == 1

    # -- forward
    def _acc(self, x, w, st, pad, sc, sh):
        a = x if sc is None else O.rne_bf16(torch.relu(x.to(F32) * sc.to(F32) + sh.to(F32)).to(F64))
        K, R, S, C = w.shape
        if "pad_tap_neighbour" in self.wrong and pad > 0:
            # the tap above the first image row reads the row before it in memory: the last row
            # of the previous image
            N, H, W, _ = a.shape
            ap = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=F64)
            ap[:, pad:pad + H, pad:pad + W] = a
            ap[1:, pad - 1, pad:pad + W] = a[:-1, H - 1]
            acc = F.conv2d(_nchw(ap), _nchw(w), stride=st, padding=0)
        else:
            acc = F.conv2d(_nchw(a), _nchw(w), stride=st, padding=pad)
        acc = _nhwc(acc)
        if "tail_k_channel" in self.wrong:
            acc = acc - torch.einsum("npq,k->npqk", O.patches(a, R, S, st, pad)[..., R - 1, S - 1, C - 1],
                                     w[:, R - 1, S - 1, C - 1].to(F64))
        return acc

    def fwd(self, x, w, st, pad, cfg=-1, stats=True, sc=None, sh=None, bm=None):
        acc = self._acc(x, w, st, pad, sc, sh)
        y = self.round(acc)
        if not stats:
            return y, None
        src = (y if "stats_from_stored" in self.wrong else acc).to(F32).reshape(-1, acc.shape[-1])
        bm = bm or 128
        mt = -(-src.shape[0] // bm)
        padded = torch.zeros(mt * bm, src.shape[1], dtype=F32)
        padded[:src.shape[0]] = src
        t = padded.reshape(mt, bm, -1)
        return y, torch.stack([t.sum(1), (t * t).sum(1)], 1).to(F64)

    def fwd_bias(self, x, w, st, pad, bias, relu):
        v = self._acc(x, w, st, pad, None, None).to(F32) + bias.to(F32)
        return self.round((torch.relu(v) if relu else v).to(F64))

    # -- data gradient
    def _dacc(self, dy, wt, H, W, st, pad):
        C, R, S, K = wt.shape
        P, Q = dy.shape[1], dy.shape[2]
        oph, opw = H - ((P - 1) * st - 2 * pad + R), W - ((Q - 1) * st - 2 * pad + S)
        if oph >= st or opw >= st:       # rows the forward never read: conv_transpose2d refuses
            return O.dgrad_acc(dy, wt, H, W, st, pad).to(F32).to(F64)
        w_kcrs = wt.permute(3, 0, 1, 2).to(F32).contiguous()
        return _nhwc(F.conv_transpose2d(_nchw(dy), w_kcrs, stride=st, padding=pad, output_padding=(oph, opw)))

    def _dfin(self, acc, addend, abits, asub):
        if addend is None:
            return self.round(acc)
        full = O.expand_addend(addend, abits, asub, acc.shape)
        add = lambda a, b: (a.to(F32) + b.to(F32)).to(F64)      # noqa: E731  (a fp32 add, as the kernel's)
        if "addend_pre" in self.wrong:
            return self.round(add(acc, full))
        return self.round(add(self.round(acc), full))

    def dgrad(self, dy, wt, H, W, st, pad, cfg=-1, addend=None, abits=None, asub=0):
        return self._dfin(self._dacc(dy, wt, H, W, st, pad), addend, abits, asub)

    def _slab(self, dx, mask, ya, ma, yb, mb, bm):
        d, terms = O.bn_terms(dx, mask, ya, ma, yb, mb)
        rows = terms.shape[1]
        bm = bm or rows
        return d, torch.stack([O.tile_rows(t, bm) for t in terms], 1)

    def dgrad_cat(self, dy, wcat, a2, bias, cfg=-1, ya=None, ma=None, bm=None):
        K, H = dy.shape[-1], dy.shape[1]
        acc = self._dacc(dy, wcat[..., :K], H, H, 1, 0) + self._dacc(a2, wcat[..., K:], H, H, 1, 0) + bias.to(F64)
        dx = self.round(acc)
        return dx, (self._slab(dx, None, ya, ma, None, None, bm)[1] if ya is not None else None)

    def dgrad_bnstat(self, dy, wt, H, W, st, pad, cfg, ya, ma, yb=None, mb=None, mask=None, addend=None, abits=None,
                     asub=0, store_masked=0, extra_rows=0, bm=None):
        dx = self._dfin(self._dacc(dy, wt, H, W, st, pad), addend, abits, asub)
        d, slab = self._slab(dx, mask, ya, ma, yb, mb, bm if st == 1 else None)
        if extra_rows:
            slab = torch.cat([slab, torch.full((extra_rows,) + slab.shape[1:], float("nan"), dtype=F64)])
        return (d if store_masked else dx), slab

    # -- weight gradient
    def wgrad(self, dy, x, R, st, pad, splits=0, cfg=-1, sink=None, layout="krsc", accumulate=True, sc=None, sh=None):
        a = x if sc is None else O.rne_bf16(torch.relu(x.to(F32) * sc.to(F32) + sh.to(F32)).to(F64))
        K, C = dy.shape[-1], x.shape[-1]
        dw = torch.nn.grad.conv2d_weight(_nchw(a), (K, C, R, R), _nchw(dy), stride=st, padding=pad)
        dw = dw.permute(0, 2, 3, 1).to(F64).contiguous()
        M = dy.shape[0] * dy.shape[1] * dy.shape[2]
        n = max(1, splits if splits > 0 else 4)
        per = -(-M // n)
        if "split_drop_pixel" in self.wrong:
            dw = dw - O.wgrad(dy, a, R, R, st, pad, pixels=(per - 1, per))
        if "dup_split" in self.wrong and per < M:
            dw = dw + O.wgrad(dy, a, R, R, st, pad, pixels=(0, per))
        if sink is not None and accumulate and "sink_overwrite" not in self.wrong:
            dw = (dw.to(F32) + sink.to(F32)).to(F64)
        return dw


# ---------------------------------------------------------------- comparison ------------------

def same(name, got, ref, ctx="", tile=None):
    """torch.equal, or the count of wrong elements and the first few as (n, h, w, channel) — for
    a 2-D quantity (row, channel) — with their (M-tile, N-tile) under ``tile`` = (bm, bn)."""
    assert got.shape == ref.shape, (name, ctx, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got)
    idx = bad.nonzero()
    lines = []
    for i in idx[:6].tolist():
        s = f"{tuple(i)}: got {got[tuple(i)].item():.9g}, ref {ref[tuple(i)].item():.9g}"
        if tile is not None and len(i) >= 2:
            row = 0
            for k, dim in zip(i[:-1], got.shape[:-1]):
                row = row * dim + k
            s += f" (M-tile {row // tile[0]}, N-tile {i[-1] // tile[1]})"
        lines.append(s)
    raise AssertionError(f"{name} {ctx}: {int(bad.sum())} of {got.numel()} elements differ; first: " + "; ".join(lines))


def _guard_fwd(d, st, pad, prologue=False, bias=False, ctx=""):
    x = O.prologue(d["x"], d["in_sc"], d["in_sh"]) if prologue else d["x"]
    unit = 0.25 if prologue else 1.0           # halves of halves: x·s + t in quarters
    a = O.fwd_acc(x.abs(), d["w"].abs(), st, pad)
    GUARD.add("fwd acc", a + (d["bias"].abs().max() if bias else 0.0), 0.5 if bias and not prologue else unit)
    return a, unit


_refs = {}


def ref_fwd(shape, regime, prologue=False):
    """The oracle's forward and its guard values, computed once per case."""
    key = ("fwd", tuple(shape), regime, prologue)
    if key not in _refs:
        d = inputs(shape, regime)
        st, pad = shape[6], shape[7]
        r = O.fwd(d["x"], d["w"], st, pad, d["in_sc"] if prologue else None, d["in_sh"] if prologue else None)
        a, unit = _guard_fwd(d, st, pad, prologue)
        # each y is exact (above), so a partial sum of Σy is bounded by Σ|y| of the real values
        GUARD.add("fwd Σ|y|", r["acc"].abs().reshape(-1, a.shape[-1]).sum(0), unit)
        r["unit"] = unit
        _refs[key] = r
    return _refs[key]


def check_fwd(impl, shape, regime, cfg=-1, prologue=False):
    """y bit-exact; Σy exact (column totals, and per tile on plain tiles); Σy² exact where the
    column's total stays below 2^24 units, else within (rows_per_tile + m_tiles)·2^-24·Σy²."""
    d = inputs(shape, regime)
    st, pad = shape[6], shape[7]
    ctx = f"(fwd {shape} {regime} cfg {cfg} prologue {prologue})"
    ref = ref_fwd(shape, regime, prologue)
    bm, bn, plain = impl.tiles("fwd", shape, cfg, in_bn=prologue)
    sc, sh = (d["in_sc"], d["in_sh"]) if prologue else (None, None)
    y, slab = impl.fwd(d["x"], d["w"], st, pad, cfg, True, sc, sh, bm=bm)
    same("y", y, ref["y"], ctx, (bm, bn))
    K = y.shape[-1]
    rows = ref["acc"].reshape(-1, K)
    same("Σy", slab[:, 0].sum(0), ref["sums"][0], ctx)
    sq, tot = slab[:, 1].sum(0), ref["sums"][1]
    exact = tot / ref["unit"] ** 2 < LIMIT
    if regime == "unit":
        assert exact.all(), f"unit regime: Σy² must be exact {ctx}"
    bound = torch.where(exact, torch.zeros_like(tot), (bm + slab.shape[0]) * U24 * tot)
    err = (sq - tot).abs()
    assert (err <= bound).all(), f"Σy² {ctx}: {int((err > bound).sum())} columns beyond the bound, first " \
                                 f"{int((err > bound).nonzero()[0])}: error {err.max().item():.6g}"
    if plain:
        same("Σy per tile", slab[:, 0], O.tile_rows(rows, bm), ctx)
        if exact.all():
            same("Σy² per tile", slab[:, 1], O.tile_rows(rows * rows, bm), ctx)
    y2, none = impl.fwd(d["x"], d["w"], st, pad, cfg, False, sc, sh)
    assert none is None
    same("y without statistics", y2, y, ctx, (bm, bn))


def check_fwd_bias(impl, shape, regime, relu):
    d = inputs(shape, regime)
    st, pad = shape[6], shape[7]
    ctx = f"(fwd_bias {shape} {regime} relu {relu})"
    _guard_fwd(d, st, pad, bias=True)
    ref = O.fwd(d["x"], d["w"], st, pad, bias=d["bias"], relu=relu)["y"]
    same("y", impl.fwd_bias(d["x"], d["w"], st, pad, d["bias"], relu), ref, ctx)


ADDENDS = ["none", "full", "masked", "compact"]


def _addend_args(d, kind):
    """-> (addend, bits, sub)"""
    return {"none": (None, None, 0), "full": (d["addend"], None, 0), "masked": (d["addend"], d["abits"], 0),
            "compact": (d["addend_c"], None, 2)}[kind]


def ref_dgrad(shape, regime, addend="none"):
    key = ("dgrad", tuple(shape), regime, addend)
    if key not in _refs:
        N, H, W, C, K, R, st, pad = shape
        d = inputs(shape, regime)
        a, bits, sub = _addend_args(d, addend)
        GUARD.add("dgrad acc", O.dgrad_acc(d["dy"].abs(), d["wt"].abs(), H, W, st, pad) + (4.0 if a is not None else 0.0))
        _refs[key] = O.dgrad(d["dy"], d["wt"], H, W, st, pad, a, bits, sub)
    return _refs[key]


def check_dgrad(impl, shape, regime, cfg=-1, addend="none"):
    N, H, W, C, K, R, st, pad = shape
    d = inputs(shape, regime)
    ctx = f"(dgrad {shape} {regime} cfg {cfg} addend {addend})"
    a, bits, sub = _addend_args(d, addend)
    bm, bn, _ = impl.tiles("dgrad", shape, cfg)
    same("dx", impl.dgrad(d["dy"], d["wt"], H, W, st, pad, cfg, a, bits, sub), ref_dgrad(shape, regime, addend), ctx,
         (bm, bn) if st == 1 else None)


def _check_slab(slab, dx_ref, mask, ya, ma, yb, mb, bm, plain, ctx, extra_rows=0):
    d, terms = O.bn_terms(dx_ref, mask, ya, ma, yb, mb)
    GUARD.add("dgrad Σ|d·(y − μ)|", terms.abs().sum(1), 0.5)
    if extra_rows:
        assert slab.shape[0] > extra_rows
        slab = slab[:slab.shape[0] - extra_rows]
    assert slab.shape[1] == terms.shape[0], (ctx, slab.shape)
    names = ("Σd", "Σd·(ya − μa)", "Σd·(yb − μb)")
    for k in range(terms.shape[0]):
        same(names[k], slab[:, k].sum(0), terms[k].sum(0), ctx)
        if plain:
            same(names[k] + " per tile", slab[:, k], O.tile_rows(terms[k], bm), ctx)
    return d


def check_dgrad_bnstat(impl, shape, regime, cfg=-1, sets=1, mask="none", addend="none", store_masked=0, extra_rows=0,
                       no_ya=False):
    """dx bit-exact (store_masked: dx·m); the slab's column totals exact, and its rows per tile
    on plain tiles; extra_rows appended rows are the caller's and are not read."""
    N, H, W, C, K, R, st, pad = shape
    d = inputs(shape, regime)
    ctx = f"(dgrad_bnstat {shape} {regime} cfg {cfg} sets {sets} mask {mask} addend {addend} " \
          f"store_masked {store_masked} extra_rows {extra_rows} no_ya {no_ya})"
    a, bits, sub = _addend_args(d, addend)
    ms = mask_of(d, mask)
    ya = None if no_ya else d["ya"]
    yb, mb = (d["yb"], d["mb"]) if sets == 2 else (None, None)
    bm, bn, plain = impl.tiles("dgrad", shape, cfg, bnstat=True)
    dx, slab = impl.dgrad_bnstat(d["dy"], d["wt"], H, W, st, pad, cfg, ya, d["ma"], yb, mb, ms, a, bits, sub,
                                 store_masked, extra_rows, bm=bm)
    dx_ref = ref_dgrad(shape, regime, addend)
    dm = _check_slab(slab, dx_ref, ms, ya, d["ma"], yb, mb, bm, plain, ctx, extra_rows)
    same("dx", dx, dm if store_masked else dx_ref, ctx, (bm, bn) if st == 1 else None)


def check_dgrad_cat(impl, case, regime, cfg=-1):
    N, H, K, K2 = case
    d = cat_inputs(case, regime)
    ctx = f"(dgrad_cat {case} {regime} cfg {cfg})"
    shape = (N, H, H, K2, K, 1, 1, 0)
    acc = O.dgrad_acc(d["dy"].abs(), d["wcat"][..., :K].abs(), H, H, 1, 0) + \
        O.dgrad_acc(d["a2"].abs(), d["wcat"][..., K:].abs(), H, H, 1, 0) + d["bias"].abs()
    GUARD.add("dgrad_cat acc", acc, 0.5)
    ref = O.dgrad(d["dy"], d["wcat"], H, H, 1, 0, cat=d["a2"], cat_bias=d["bias"])
    bm, bn, plain = impl.tiles("dgrad", shape, cfg, cat_ch=K2)
    dx, none = impl.dgrad_cat(d["dy"], d["wcat"], d["a2"], d["bias"], cfg)
    assert none is None
    same("dx", dx, ref, ctx, (bm, bn))
    bm, bn, plain = impl.tiles("dgrad", shape, cfg, cat_ch=K2, bnstat=True)
    dx2, slab = impl.dgrad_cat(d["dy"], d["wcat"], d["a2"], d["bias"], cfg, d["ya"], d["ma"], bm=bm)
    same("dx with statistics", dx2, ref, ctx, (bm, bn))
    _check_slab(slab, ref, None, d["ya"], d["ma"], None, None, bm, plain, ctx)


def ref_wgrad(shape, regime, prologue=False):
    key = ("wgrad", tuple(shape), regime, prologue)
    if key not in _refs:
        N, H, W, C, K, R, st, pad = shape
        d = inputs(shape, regime)
        sc, sh = (d["in_sc"], d["in_sh"]) if prologue else (None, None)
        x = O.prologue(d["x"], sc, sh) if prologue else d["x"]
        GUARD.add("wgrad acc", O.wgrad(d["dy"].abs(), x.abs(), R, R, st, pad) + 8.0, 0.25 if prologue else 1.0)
        _refs[key] = O.wgrad(d["dy"], d["x"], R, R, st, pad, sc, sh)
    return _refs[key]


def check_wgrad(impl, shape, regime, cfg=-1, splits=0, sink=None, prologue=False, accumulate=True):
    """dW bit-exact; sink: None | "krsc" | "cl" (the sink's layout), accumulated into (or, with
    accumulate off, overwritten)."""
    N, H, W, C, K, R, st, pad = shape
    d = inputs(shape, regime)
    ctx = f"(wgrad {shape} {regime} cfg {cfg} splits {splits} sink {sink} prologue {prologue} acc {accumulate})"
    ref = ref_wgrad(shape, regime, prologue)
    if sink is not None and accumulate:
        ref = ref + d["sink"]
    sc, sh = (d["in_sc"], d["in_sh"]) if prologue else (None, None)
    got = impl.wgrad(d["dy"], d["x"], R, st, pad, splits, cfg, d["sink"] if sink else None, sink or "krsc", accumulate,
                     sc, sh)
    same("dW", got, ref, ctx)


def short_split(steps, unit=1):
    """A split request whose normalised last split is short (None if the steps allow none)."""
    for req in range(2, 9):
        per = -(-(-(-steps // req)) // unit) * unit
        n = -(-steps // per)
        if n > 1 and steps % per != 0:
            return req
    return None


def wgrad_variants(impl_or_none, shape, cfg, steps, unit=1):
    """The (splits, sink) runs of one weight-gradient row: direct, a short last split, auto, and
    accumulation into an integer sink."""
    runs = [(1, None), (0, None), (0, "krsc"), (1, "krsc")]
    s = short_split(steps, unit)
    if s is not None:
        runs += [(s, None), (s, "krsc")]
    return runs


class knob:
    """``with knob(m, "wgrad1x1_big_set", 2):`` — a setter of the extension, restored on exit."""

    def __init__(self, m, name, value):
        self.m, self.name, self.value = m, name, value

    def __enter__(self):
        self.prev = getattr(self.m, self.name)(self.value) if self.name else None

    def __exit__(self, *exc):
        if self.name:
            getattr(self.m, self.name)(self.prev)


# ---------------------------------------------------------------- deferred reductions ---------
DEFER_JOBS = [(_w3(1, 16, 64, 128, 1), 9), (_w1(1, 8, 128, 128, 1), 10), ((2, 9, 7, 128, 64, 3, 1, 1), 0),
              ((4, 8, 8, 8, 24, 1, 1, 0), 3)]


class deferring:
    """Queue the split-K reductions of the wgrads launched inside, on a stream of its own (the
    null stream never defers); on exit cancel, synchronize, release the kept slabs."""

    def __init__(self, impl):
        self.impl = impl

    def __enter__(self):
        self.stream = torch.cuda.Stream(self.impl.dev)
        self.stream.wait_stream(torch.cuda.current_stream(self.impl.dev))
        self.ctx = torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        self.impl.m.splitk_defer_begin()
        return self

    def __exit__(self, *exc):
        try:
            self.impl.m.splitk_defer_cancel()
        finally:
            self.ctx.__exit__(*exc)
            torch.cuda.synchronize()
            self.impl.m.side_stash_release()


def _dev_wgrad(impl, shape, cfg, regime, sink, accumulate, splits=2):
    N, H, W, C, K, R, st, pad = shape
    d = inputs(shape, regime)
    impl.m.conv_wgrad(impl._b(d["dy"]), impl._b(d["x"]), R, R, st, pad, splits, cfg, sink, accumulate)


def check_defer_mixed(impl, regime):
    """Four wgrads of different families and sizes into distinct sinks, one flush: the oracle's
    dW + sink, and the same four launched undeferred."""
    sinks = [inputs(s, regime)["sink"].to(F32).to(impl.dev) for s, _ in DEFER_JOBS]
    plain = [t.clone() for t in sinks]
    for (s, cfg), t in zip(DEFER_JOBS, plain):
        assert plan(impl.m, "wgrad", s, cfg, splits=2, accumulate=True)["splits"] == 2
        _dev_wgrad(impl, s, cfg, regime, t, True)
    with deferring(impl):
        for (s, cfg), t in zip(DEFER_JOBS, sinks):
            _dev_wgrad(impl, s, cfg, regime, t, True)
        impl.m.splitk_defer_flush()
        torch.cuda.synchronize()
    for (s, cfg), t, u in zip(DEFER_JOBS, sinks, plain):
        ref = ref_wgrad(s, regime) + inputs(s, regime)["sink"]
        same("deferred dW", t.cpu().to(F64), ref, f"(mixed queue {s} cfg {cfg} {regime})")
        same("undeferred dW", u.cpu().to(F64), ref, f"(mixed queue {s} cfg {cfg} {regime})")


def check_defer_duplicate(impl, regime):
    """The same sink queued twice, accumulating: the second request flushes the first, and the
    sink ends at prior + 2·dW."""
    s, cfg = DEFER_JOBS[2]
    t = inputs(s, regime)["sink"].to(F32).to(impl.dev)
    with deferring(impl):
        _dev_wgrad(impl, s, cfg, regime, t, True)
        _dev_wgrad(impl, s, cfg, regime, t, True, splits=3)
        impl.m.splitk_defer_flush()
        torch.cuda.synchronize()
    GUARD.add("duplicate sink", 2 * O.wgrad(inputs(s, regime)["dy"].abs(), inputs(s, regime)["x"].abs(), 3, 3, 1, 1) + 8)
    same("sink", t.cpu().to(F64), 2 * ref_wgrad(s, regime) + inputs(s, regime)["sink"], f"(duplicate sink {regime})")


def check_defer_full(impl, regime, jobs=18):
    """18 jobs: the queue fills at 16, is issued, and goes on; every sink right."""
    work = [DEFER_JOBS[i % len(DEFER_JOBS)] for i in range(jobs)]
    sinks = [inputs(s, regime)["sink"].to(F32).to(impl.dev) for s, _ in work]
    with deferring(impl):
        for i, ((s, cfg), t) in enumerate(zip(work, sinks)):
            _dev_wgrad(impl, s, cfg, regime, t, i % 2 == 0)
        impl.m.splitk_defer_flush()
        torch.cuda.synchronize()
    for i, ((s, cfg), t) in enumerate(zip(work, sinks)):
        ref = ref_wgrad(s, regime) + (inputs(s, regime)["sink"] if i % 2 == 0 else 0.0)
        same("dW", t.cpu().to(F64), ref, f"(full queue job {i} {s} cfg {cfg} {regime})")


def check_defer_empty(impl):
    with deferring(impl):
        impl.m.splitk_defer_flush()          # nothing queued: no launch
        impl.m.splitk_defer_flush()          # not deferring any more: still nothing
    s, cfg = DEFER_JOBS[3]
    check_wgrad(impl, s, "unit", cfg, 2)     # and the plain path is intact afterwards


# ---------------------------------------------------------------- environment-knob children ---
CHILD_SETS = {
    "merge0": ({"SDX_DGRAD_MERGE": "0"}, dict(merged=False)),
    "merge1": ({"SDX_DGRAD_MERGE": "1"}, dict(merged=True)),
    "glds0": ({"SDX_IGEMM_GLDS": "0"}, dict(fwd_depth=(1, 2), wgrad_depth=(1, 2))),
    "glds2": ({"SDX_IGEMM_GLDS": "2"}, dict(fwd_depth=(3, 6), wgrad_depth=(3,))),
}
CHILD_SHAPES = [FWD_CASES[k] for k in ("ragged M, 18 K-tiles", "merged classes", "strided 1x1", "odd stride 2",
                                       "odd stride 3")]
CHILD_MARKER = "CONV-KNOBS-OK"


def run_child_list(impl):
    for shape in CHILD_SHAPES:
        for regime in REGIMES:
            check_fwd(impl, shape, regime)
            check_dgrad(impl, shape, regime)
            check_dgrad_bnstat(impl, shape, regime, mask="bits")
            for splits in (1, 3, 0):
                check_wgrad(impl, shape, regime, -2, splits)


def _child(name):
    import signal
    signal.alarm(240)       # the child's own limit: SIGALRM ends it
    env, expect = CHILD_SETS[name]
    assert all(os.environ.get(k) == v for k, v in env.items()), "knob not set"
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    if "merged" in expect:      # a strided 1x1 is merged only under =1, a strided 3x3 not under =0
        for key in ("merged classes", "strided 1x1"):
            assert plan(m, "dgrad", FWD_CASES[key])["merged"] == expect["merged"], (name, key)
    else:
        for shape in CHILD_SHAPES:
            assert all(dp in expect["fwd_depth"] for dp in plan(m, "fwd", shape)["depth"]), (name, shape)
            assert plan(m, "wgrad", shape, -2)["depth"] in expect["wgrad_depth"], (name, shape)
    run_child_list(ExtImpl(m, torch.device("cuda:0")))
    torch.cuda.synchronize()
    print(CHILD_MARKER)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
