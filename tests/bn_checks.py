"""Cases, inputs, bounds and comparison functions of the BatchNorm oracle tests.

The comparison functions take an *implementation*: an object with one method per BatchNorm
operation that maps CPU tensors to CPU tensors. ``ExtImpl`` runs the HIP kernels of the
extension; ``TwinImpl`` runs the fp32 twin of tests/bn_oracle.py (optionally with a deliberate
defect). tests/test_bn_oracle.py holds the twin to the bounds on the CPU,
tests/test_gpu_bn_oracle.py holds the kernels to the same bounds, and ``python -m bn_checks
--child`` is the fresh process of the knob test.

Bounds (u8 = 2^-8: one bf16 rounding, u24 = 2^-24: one fp32 rounding, u52 = 2^-52):

  column reduction     |got − ref| <= rows·u52·Σ|v|                    fp64 sum of fp32 values
  finalize             mean, invstd: u24·|ref| (one cast)     scale: 2·u24·|ref| (cast, product)
                       shift: 4·u24·(|β| + |mean·γ·invstd|)   (two casts, two products, one sum)
                       running: 4·u24·(|(1−m)·old| + |m·new|) (1−m, two products, a cast, a sum)
  bn_apply             |out − z| <= u8·|z| + 2^-22·T           a fp32 chain of <= 4 roundings of
                                                               magnitudes <= T, fused or not
  bn_bwd_reduce        (n_t + 3)·u24·Σ|term|                   y−μ, the product, n_t fp32 adds per
                                                               thread, the fp32 partial
  bn_bwd_coef          A, D, E: u24·|ref| (+ 1e-15·(|A·Σdz/n| + |D·μ|) for E: its fp64 sum cancels)
                       dγ, dβ: 2·u24·(|new| + |sink|)          a cast and a fp32 add
  bn_bwd_apply         u8·|z| + 2^-22·(|A·dz| + |D·y| + |E|);  dz bit-equal
  bn_eval_affine       EVAL_AFFINE_TOL (measured, see below)

A mask recomputed from the BN input (``ya·msc + msh > 0``) is decided by a fp32 value in the
kernel and by a fp64 value in the oracle. The tests make no allowance for that: dz is bit-equal
and the reduce bound is the one above for this mask source too. ``mask_margin_ok`` states what
makes this sound, and tests/test_bn_oracle.py asserts it for every case: each generated value
is either exactly 0 (both terms 0, in any arithmetic) or farther from 0 than a fp32 evaluation
can move it.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

import bn_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U8, U22, U24, U52 = 2.0 ** -8, 2.0 ** -22, 2.0 ** -24, 2.0 ** -52
EPS, MOMENTUM = 1e-5, 0.1

# bn_eval_affine uses rsqrtf, whose error bound the project does not record. Largest relative
# error of scale (against |ref|) and shift (against |β| + |mean·γ·invstd|) measured on an MI355X
# against the fp64 oracle over EVAL_CASES (docs/PARITY.md); the tolerance is twice that, at
# least 2·u24, and the test refuses a measured value that would need more than 8·u24.
EVAL_AFFINE_MEASURED = 2.27 * U24
EVAL_AFFINE_TOL = max(2.0 * EVAL_AFFINE_MEASURED, 2.0 * U24)
EVAL_AFFINE_CEILING = 8.0 * U24
assert EVAL_AFFINE_TOL <= EVAL_AFFINE_CEILING

# ---------------------------------------------------------------- mirrors of the grid rules ---


def _env_int(name):
    try:
        return int(os.environ.get(name, "0"))
    except ValueError:
        return 0


def ew_cap(bwd=False):
    """bn.hip ew_grid (lines 597-613), the env_cap lambda: a knob below 8 is ignored, else it
    is rounded down to a multiple of 8; SDX_EW_BLOCKS_BWD defaults to the forward cap."""
    def cap(name, dflt):
        v = _env_int(name)
        return v // 8 * 8 if v >= 8 else dflt
    fwd = cap("SDX_EW_BLOCKS", 2048)
    return cap("SDX_EW_BLOCKS_BWD", fwd) if bwd else fwd


def ew_grid(n8, bwd=False):
    """bn.hip ew_grid (lines 597-613) with SDX_EW_UNROLL = 1: ceil(n8 / 256) blocks in [1, cap]."""
    return max(1, min((n8 + 255) // 256, ew_cap(bwd)))


def ew_path(C, rows, bwd=False):
    """-> (fast, min_iters, max_iters): the branch of bn_apply_kernel / bn_bwd_apply_kernel
    (bn.hip lines 350 and 570: fast iff the grid stride is a multiple of C/8) and the fewest /
    most grid-stride iterations of a thread."""
    n8, C8 = rows * C // 8, C // 8
    stride = ew_grid(n8, bwd) * 256
    return stride % C8 == 0, n8 // stride, -(-n8 // stride)


def col_reduce_gy(rows):
    """bn.hip col_reduce_gy (lines 617-629): int(sqrt(rows)·scale + 0.5) in [1, 64], scale =
    SDX_CR_GY when positive, else 0.5."""
    try:
        scale = float(os.environ.get("SDX_CR_GY", "0"))
    except ValueError:
        scale = 0.0
    if not scale > 0.0:
        scale = 0.5
    return max(1, min(64, int(math.sqrt(rows) * scale + 0.5)))


def col_reduce_per(rows):
    """Rows per block of col_reduce_kernel (bn.hip line 174)."""
    return -(-rows // col_reduce_gy(rows))


def bn_bwd_reduce_blocks(numel):
    """bn.hip bn_bwd_reduce_blocks (lines 708-715): ceil(n8 / 4096) in [1, 1024]."""
    return max(1, min(1024, (numel // 8 + 4095) // 4096))


def reduce_n_t(rows, C):
    """Chunks one thread of bn_bwd_reduce_kernel accumulates in fp32 (bn.hip line 452)."""
    n8 = rows * C // 8
    return -(-n8 // (256 * bn_bwd_reduce_blocks(rows * C)))


# ---------------------------------------------------------------- case tables -----------------
# (C, rows): the smallest shapes at which each edge exists; test_bn_oracle.py asserts the path
# each one is meant to hit with the mirrors above.
EW_CASES = [(8, 5), (16, 33), (24, 100), (24, 256), (40, 77), (136, 31), (2048, 3), (4096, 2),
            (1024, 5 * 33 * 31), (24, 250000)]
REDUCE_CASES = [(8, 5), (16, 33), (64, 1), (512, 9), (1024, 7), (2048, 1), (2048, 3), (128, 4097)]
# The 3-set column reduction (col_reduce_kernel<3, *>) sees the partial slab of bn_bwd_reduce,
# whose row count is the block count g = ceil(n8 / 4096). These shapes (two BN sets) put g on the
# row table of the column reduction: n8 = 4096·(g − 1) + 1 (C = 8) or + 8 (C = 64), a ragged
# last stride with n_t = 11 .. 16. g = 197 is the smallest with more than 28 rows per block, where the
# first thread row takes the 32-row unrolled trip with three sets (6.4 M elements). The trip's
# tail (g = 257: 8.4 M elements) and gy = 64 (g >= 16129; g is capped at 1024) are out of reach.
REDUCE3_G = [3, 4, 5, 8, 9, 31, 32, 33, 36, 37, 127, 128, 197]


def reduce3_case(g):
    """(C, rows) with bn_bwd_reduce_blocks == g; C alternates between one thread folding the
    block (C = 8) and 32 threads per channel group (C = 64)."""
    return (8, 4096 * (g - 1) + 1) if g % 2 else (64, 512 * (g - 1) + 1)


REDUCE3_CASES = [reduce3_case(g) for g in REDUCE3_G]
# rows of the column reduction. 196/197 and 224/257: 28/29 and 32/33 rows per block, the first
# and last thread row entering the 32-row unrolled trip, and one row of tail after it.
STATS_ROWS = [1, 3, 4, 5, 8, 9, 31, 32, 33, 36, 37, 127, 128, 196, 197, 224, 257]
STATS_ROWS_MAXY = [16128, 16129]          # gy 63 -> 64, C = 72 only
STATS_C = [8, 40, 64, 72, 200, 4096]      # 4096 with rows <= 33
EVAL_CASES = [8, 40, 64, 200, 4096]
MASK_KINDS = ["none", "act", "bits", "affine"]
SMALL_ROWS = 4097                          # the knob child runs the cases up to this many rows
# With SDX_EW_BLOCKS=8 / SDX_EW_BLOCKS_BWD=16 no case of the tables above reaches a second
# grid-stride iteration (n8 <= 2048 for all of them), so the elementwise kernels also get two
# shapes that do under the knobs: fallback branch with 4-5 (forward) and 2-3 (backward)
# iterations, and fast branch with 3-4 and 1-2. (At the default cap both take one iteration.)
EW_KNOB_CASES = [(24, 3000), (64, 1000)]


def stats_rows_for(C):
    rows = [r for r in STATS_ROWS if C != 4096 or r <= 33]
    return rows + (STATS_ROWS_MAXY if C == 72 else [])


# ---------------------------------------------------------------- inputs ----------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * p for k, p in zip(key, (1000003, 10007, 101))) % (2 ** 31))
    return g


def channel_vectors(C, g):
    """scale in ±[0.5, 1.5], shift and mean ~ N(0, 1): neighbouring channels differ by far more
    than any tolerance."""
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    return (sign * (torch.rand(C, generator=g) + 0.5)).to(F32), torch.randn(C, generator=g), torch.randn(C, generator=g)


def _with_zeros(x, g):
    """5 % exact +0 and 5 % exact −0."""
    u = torch.rand(x.shape, generator=g)
    x = torch.where(u < 0.05, torch.zeros(()), x)
    return torch.where((u >= 0.05) & (u < 0.10), -torch.zeros(()), x)


_inputs = {}


def inputs(C, rows):
    """All tensors of one (C, rows) case, generated once per process and never modified."""
    if (C, rows) in _inputs:
        return _inputs[(C, rows)]
    g = _gen(C, rows)
    d = {"C": C, "rows": rows}
    d["y"] = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(BF16)
    d["r"] = (torch.randn(rows, C, generator=g) - 1).to(BF16)
    d["sc"], d["sh"], d["mu_a"] = channel_vectors(C, g)
    d["sc2"], d["sh2"], d["mu_b"] = channel_vectors(C, g)
    # forward edge: exact ±0 in y, and a shift of −0 (channels 3, 10, ...) or +0 (5, 12, ...), so
    # that y·sc + sh is exactly 0 there and, with ReLU off, −0 where y·sc = −0 and sh = −0: the
    # output is a zero and its mask bit is clear. (A generator of its own: the other draws stay.)
    d["y"] = _with_zeros(d["y"].float(), _gen(C, rows, 3)).to(BF16)
    ch = torch.arange(C) % 7
    d["sh"] = torch.where(ch == 3, -torch.zeros(()), torch.where(ch == 5, torch.zeros(()), d["sh"]))
    d["out"] = _with_zeros(torch.randn(rows, C, generator=g), g).to(BF16)
    d["dout"] = _with_zeros(torch.randn(rows, C, generator=g), g).to(BF16)
    # BN inputs of the backward: exact zeros in ya and a zero msh in every fifth channel, so
    # that ya·msc + msh is exactly 0 there (the mask must be clear)
    d["ya"] = _with_zeros(torch.randn(rows, C, generator=g) * 2 + 0.5, g).to(BF16)
    d["yb"] = (torch.randn(rows, C, generator=g) - 1).to(BF16)
    d["msc"], msh, _ = channel_vectors(C, g)
    d["msh"] = torch.where(torch.arange(C) % 5 == 0, torch.zeros(()), msh)
    d["bits"] = torch.from_numpy(O.relu_bits(d["out"]))
    d["g_a"], _, _ = channel_vectors(C, g)
    d["g_b"], _, _ = channel_vectors(C, g)
    d["inv_a"] = torch.rand(C, generator=g) + 0.5
    d["inv_b"] = torch.rand(C, generator=g) + 0.5
    coefs = []
    for _ in range(2):
        A, E, _ = channel_vectors(C, g)
        D, _, _ = channel_vectors(C, g)
        coefs.append(torch.stack([A, D * 0.25, E]).contiguous())
    d["ca"], d["cb"] = coefs
    d["sinks"] = [torch.randn(C, generator=g) for _ in range(4)]
    _inputs[(C, rows)] = d
    return d


def mask_source(d, kind):
    return {"none": None, "act": ("act", d["out"]), "bits": ("bits", d["bits"]),
            "affine": ("affine", d["msc"], d["msh"])}[kind]


_slabs = {}


def stat_slab(rows, C):
    """[rows, 2, C] float32 conv-epilogue statistics of 16 values per slab row: Σ of mixed
    magnitudes 1e-3 .. 1e4 within a column (a fp32 reduction would miss the bound), and a Σ²
    column with Σ²_i >= Σ_i² / 16, so that the variance is non-negative for any count >= 16·rows."""
    if (rows, C) not in _slabs:
        g = _gen(rows, C, 17)
        a = torch.randn(rows, C, generator=g) * 10.0 ** (torch.rand(rows, C, generator=g) * 7 - 3)
        q = a.double() ** 2 / 16 * (1 + torch.rand(rows, C, generator=g).double()) + 1e-3
        _slabs[(rows, C)] = torch.stack([a.to(F32), q.to(F32)], 1).contiguous()
    return _slabs[(rows, C)]


# ---------------------------------------------------------------- implementations -------------

class TwinImpl:
    """The fp32 twin behind the implementation interface; ``wrong`` names deliberate defects."""

    def __init__(self, wrong=()):
        self.wrong = set(wrong)

    def stats_reduce(self, slab):
        return O.twin_col_reduce(slab, self.wrong)

    def finalize(self, sums, count, gamma, beta, eps, mom, rm=None, rv=None):
        return O.twin_finalize(sums, count, gamma, beta, eps, mom, rm, rv, self.wrong)

    def stats_finalize(self, slab, count, gamma, beta, eps, mom, rm=None, rv=None):
        return self.finalize(self.stats_reduce(slab), count, gamma, beta, eps, mom, rm, rv)

    def eval_affine(self, gamma, beta, rm, rv, eps):
        return O.twin_eval_affine(gamma, beta, rm, rv, eps)

    def apply(self, y, sc, sh, r, sc2, sh2, res_mode, relu, want_mask):
        out = O.twin_apply(y, sc, sh, r, sc2, sh2, res_mode, relu, self.wrong)
        return out, (O.relu_bits(out) if want_mask else None)

    def bwd_reduce(self, dout, ms, ya, mu_a, yb=None, mu_b=None):
        return O.twin_bwd_sums(dout, ms, ya, mu_a, yb, mu_b, bn_bwd_reduce_blocks(dout.numel()), self.wrong)

    def bwd_coef(self, sums, count, g_a, mu_a, inv_a, g_b=None, mu_b=None, inv_b=None, sinks=None, grad_scale=1.0):
        s = sinks or [None] * 4
        a = O.twin_coef(sums, count, g_a, mu_a, inv_a, grad_scale, 0, s[0], s[1], self.wrong)
        o = dict(ca=a["coef"], dga=a["dgamma"], dba=a["dbeta"], cb=None, dgb=None, dbb=None)
        if sums.shape[0] == 3:
            b = O.twin_coef(sums, count, g_b, mu_b, inv_b, grad_scale, 1, s[2], s[3], self.wrong)
            o.update(cb=b["coef"], dgb=b["dgamma"], dbb=b["dbeta"])
        return o

    def bwd_reduce_coef(self, dout, ms, ya, mu_a, yb, mu_b, count, g_a, inv_a, g_b=None, inv_b=None, sinks=None):
        return self.bwd_coef(self.bwd_reduce(dout, ms, ya, mu_a, yb, mu_b), count, g_a, mu_a, inv_a, g_b, mu_b,
                             inv_b, sinks)

    def bwd_apply(self, dout, ms, ya, ca, yb=None, cb=None, want_dz=True):
        o = O.twin_bwd_apply(dout, ms, ya, ca, yb, cb, self.wrong)
        if not want_dz:
            o["dz"] = None
        return o


class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _a(self, t):       # [rows, C] bf16 -> NHWC on the device
        return None if t is None else t.to(BF16).reshape(1, 1, *t.shape).to(self.dev)

    def _v(self, t, dtype=F32):
        return None if t is None else t.to(dtype).contiguous().to(self.dev)

    def _mask_args(self, ms):
        """-> (outv, msc, msh)"""
        if ms is None:
            return None, None, None
        if ms[0] == "act":
            return self._a(ms[1]), None, None
        if ms[0] == "bits":
            return ms[1].to(self.dev), None, None
        return None, self._v(ms[1]), self._v(ms[2])

    @staticmethod
    def _back(t, shape):
        return t.cpu().reshape(shape).float()

    def stats_reduce(self, slab):
        return self.m.bn_stats_reduce(slab.to(self.dev)).cpu()

    def _fin(self, fn, first, count, gamma, beta, eps, mom, rm, rv):
        rm, rv = self._v(rm), self._v(rv)
        r = fn(first.to(self.dev), float(count), self._v(gamma), self._v(beta), eps, mom, rm is not None, rm, rv)
        o = dict(zip(("scale", "shift", "mean", "invstd"), (t.cpu() for t in r)))
        if rm is not None:
            o.update(running_mean=rm.cpu(), running_var=rv.cpu())
        return o

    def finalize(self, sums, count, gamma, beta, eps, mom, rm=None, rv=None):
        return self._fin(self.m.bn_finalize, sums, count, gamma, beta, eps, mom, rm, rv)

    def stats_finalize(self, slab, count, gamma, beta, eps, mom, rm=None, rv=None):
        return self._fin(self.m.bn_stats_finalize, slab, count, gamma, beta, eps, mom, rm, rv)

    def eval_affine(self, gamma, beta, rm, rv, eps):
        sc, sh = self.m.bn_eval_affine(self._v(gamma), self._v(beta), self._v(rm), self._v(rv), eps)
        return sc.cpu(), sh.cpu()

    def apply(self, y, sc, sh, r, sc2, sh2, res_mode, relu, want_mask):
        mask = torch.full((y.numel() // 8,), 0xA5, dtype=torch.uint8, device=self.dev) if want_mask else None
        out = self.m.bn_apply(self._a(y), self._v(sc), self._v(sh), self._a(r) if res_mode else None,
                              self._v(sc2) if res_mode == 1 else None, self._v(sh2) if res_mode == 1 else None,
                              res_mode, relu, mask_out=mask)
        return self._back(out, y.shape), (mask.cpu().numpy() if want_mask else None)

    def bwd_reduce(self, dout, ms, ya, mu_a, yb=None, mu_b=None):
        outv, msc, msh = self._mask_args(ms)
        return self.m.bn_bwd_reduce(self._a(dout), outv, self._a(ya), self._v(mu_a), self._a(yb), self._v(mu_b),
                                    msc=msc, msh=msh).cpu()

    @staticmethod
    def _coef_out(r, sinks, two):
        o = dict(ca=r[0].cpu(), dga=r[2].cpu(), dba=r[3].cpu(), cb=None, dgb=None, dbb=None)
        if two:
            o.update(cb=r[1].cpu(), dgb=r[4].cpu(), dbb=r[5].cpu())
        return o

    def _sinks(self, sinks, two):
        if sinks is None:
            return {}
        s = [self._v(t).clone() for t in sinks[:4 if two else 2]]
        return dict(zip(("sink_ga", "sink_ba", "sink_gb", "sink_bb"), s))

    def bwd_coef(self, sums, count, g_a, mu_a, inv_a, g_b=None, mu_b=None, inv_b=None, sinks=None, grad_scale=1.0):
        two = sums.shape[0] == 3
        r = self.m.bn_bwd_coef(self._v(sums, F64), float(count), self._v(g_a), self._v(mu_a), self._v(inv_a),
                               self._v(g_b), self._v(mu_b), self._v(inv_b), grad_scale=grad_scale,
                               **self._sinks(sinks, two))
        return self._coef_out(r, sinks, two)

    def bwd_reduce_coef(self, dout, ms, ya, mu_a, yb, mu_b, count, g_a, inv_a, g_b=None, inv_b=None, sinks=None):
        outv, msc, msh = self._mask_args(ms)
        two = yb is not None
        r = self.m.bn_bwd_reduce_coef(self._a(dout), outv, self._a(ya), self._v(mu_a), self._a(yb), self._v(mu_b),
                                      msc, msh, float(count), self._v(g_a), self._v(inv_a), self._v(g_b),
                                      self._v(inv_b), **self._sinks(sinks, two))
        return self._coef_out(r, sinks, two)

    def bwd_apply(self, dout, ms, ya, ca, yb=None, cb=None, want_dz=True):
        outv, msc, msh = self._mask_args(ms)
        dya, dyb, dz = self.m.bn_bwd_apply(self._a(dout), outv, self._a(ya), self._v(ca), self._a(yb), self._v(cb),
                                           want_dz, msc=msc, msh=msh)
        assert dz.numel() == (dout.numel() if want_dz else 0)
        assert dyb.numel() == (dout.numel() if yb is not None else 0)
        return dict(dya=self._back(dya, dout.shape), dyb=self._back(dyb, dout.shape) if yb is not None else None,
                    dz=self._back(dz, dout.shape) if want_dz else None)


# ---------------------------------------------------------------- comparison ------------------

def within(stats, name, got, ref, bound, where=None, ctx=""):
    """Assert |got − ref| <= bound elementwise (optionally only where ``where``); record the
    largest error / bound under ``name`` in ``stats`` (0/0 counts as 0)."""
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite result {ctx}"
    err = (got - ref).abs()
    if where is not None:
        err = torch.where(where, err, torch.zeros((), dtype=F64))
    ratio = torch.where(err == 0, torch.zeros((), dtype=F64), err / bound)
    worst = ratio.max().item() if ratio.numel() else 0.0
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), worst)
    if not worst <= 1.0:
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{name} {ctx}: error / bound = {worst:.4g} at flat index {i}: got "
                             f"{got.reshape(-1)[i].item():.9g}, ref {ref.reshape(-1)[i].item():.9g}, "
                             f"bound {bound.reshape(-1)[i].item():.4g}")


def same_bits(name, a, b, ctx=""):
    assert a.shape == b.shape, (name, a.shape, b.shape)
    assert np.array_equal(a.contiguous().numpy().view(np.uint8), b.contiguous().numpy().view(np.uint8)), \
        f"{name}: not bit-equal {ctx}"


def check_apply(impl, C, rows, stats=None, modes=(0, 1, 2), relus=(True, False)):
    d = inputs(C, rows)
    for res_mode in modes:
        z0, T = O.apply(d["y"], d["sc"], d["sh"], d["r"], d["sc2"], d["sh2"], res_mode, relu=False)
        sure = ((z0.abs() > U22 * T) | (T == 0)).reshape(-1).numpy()     # T == 0: exactly 0, bit clear
        ref_bits = O.unpack_bits(O.relu_bits(z0), z0.numel()).numpy()
        for relu in relus:
            ctx = f"(C={C}, rows={rows}, res_mode={res_mode}, relu={relu})"
            z = z0.clamp_min(0.0) if relu else z0
            out, bits = impl.apply(d["y"], d["sc"], d["sh"], d["r"], d["sc2"], d["sh2"], res_mode, relu, True)
            within(stats, "bn_apply", out, z, U8 * z.abs() + U22 * T, ctx=ctx)
            assert np.array_equal(bits, O.relu_bits(out)), f"bn_apply mask != bits of its own output {ctx}"
            got_bits = O.unpack_bits(bits, z0.numel()).numpy()
            assert np.array_equal(got_bits[sure], ref_bits[sure]), f"bn_apply mask != oracle mask {ctx}"
            out2, none = impl.apply(d["y"], d["sc"], d["sh"], d["r"], d["sc2"], d["sh2"], res_mode, relu, False)
            assert none is None
            same_bits("bn_apply without mask_out", out, out2, ctx)


def mask_margin_ok(d):
    """True iff every value ya·msc + msh of the case has the same sign in fp32, fused or not, as
    in fp64: both terms are exactly 0, or |v| exceeds u24·|ya·msc|, the most a rounded product
    can move the sum (the rounding of the sum itself keeps the sign)."""
    p = d["ya"].to(F64) * d["msc"].to(F64)
    v = p + d["msh"].to(F64)
    return bool((((p == 0) & (d["msh"].to(F64) == 0)) | (v.abs() > U24 * p.abs())).all())


def check_bwd_apply(impl, C, rows, stats=None, kinds=MASK_KINDS, sets=(False, True)):
    d = inputs(C, rows)
    for kind in kinds:
        ms = mask_source(d, kind)
        for two in sets:
            ctx = f"(C={C}, rows={rows}, mask={kind}, two={two})"
            yb, cb = (d["yb"], d["cb"]) if two else (None, None)
            ref = O.bwd_apply(d["dout"], ms, d["ya"], d["ca"], yb, cb)
            got = impl.bwd_apply(d["dout"], ms, d["ya"], d["ca"], yb, cb, True)
            assert np.array_equal(O.bf16_bits(got["dz"]), O.bf16_bits(ref["dz"])), \
                f"bn_bwd_apply dz not bit-equal {ctx}"
            for key in ("a", "b") if two else ("a",):
                zz, T = ref["dy" + key], ref["T" + key]
                within(stats, "bn_bwd_apply", got["dy" + key], zz, U8 * zz.abs() + U22 * T, ctx=ctx)
            got0 = impl.bwd_apply(d["dout"], ms, d["ya"], d["ca"], yb, cb, False)
            assert got0["dz"] is None
            same_bits("bn_bwd_apply dya without dz", got["dya"], got0["dya"], ctx)
            if two:
                same_bits("bn_bwd_apply dyb without dz", got["dyb"], got0["dyb"], ctx)


def reduce_bound(d, abs_sums):
    """(n_t + 3)·u24·Σ|term|"""
    return (reduce_n_t(d["rows"], d["C"]) + 3) * U24 * abs_sums


def coef_bounds(c, sink_g, sink_b, count, inv, mu, grad_scale, dsdz=None, dsdzy=None):
    """Bounds of one BN set's (A, D, E, dγ, dβ) around the oracle's ``c``; dsdz / dsdzy: the
    bounds of the sums the coefficients were computed from (None: exact fp64 sums)."""
    inv, mu = inv.to(F64), mu.to(F64)
    zero = torch.zeros_like(inv)
    dsdz = zero if dsdz is None else dsdz
    dsdzy = zero if dsdzy is None else dsdzy
    sg = zero if sink_g is None else sink_g.to(F64).abs()
    sb = zero if sink_b is None else sink_b.to(F64).abs()
    dD = (c["A"] * inv * inv / count).abs() * dsdzy
    dE = (c["A"] / count).abs() * dsdz + mu.abs() * dD
    dg, db = (inv * grad_scale).abs() * dsdzy, abs(grad_scale) * dsdz
    return dict(A=U24 * c["A"].abs(), D=U24 * (c["D"].abs() + dD) + dD,
                E=U24 * (c["E"].abs() + dE) + dE + 1e-15 * (c["E_terms"] + dE),
                dgamma=2 * U24 * (c["dgamma"].abs() + dg + sg) + dg,
                dbeta=2 * U24 * (c["dbeta"].abs() + db + sb) + db)


def _check_coef_result(stats, name, got, d, sums, count, two, sinks, grad_scale, dS, ctx):
    for si, (key, g, mu, inv) in enumerate((("a", d["g_a"], d["mu_a"], d["inv_a"]),
                                            ("b", d["g_b"], d["mu_b"], d["inv_b"]))[:2 if two else 1]):
        c = O.coef(sums, count, g, mu, inv, grad_scale, si)
        sk = (None, None) if sinks is None else (sinks[2 * si], sinks[2 * si + 1])
        b = coef_bounds(c, sk[0], sk[1], count, inv, mu, grad_scale,
                        None if dS is None else dS[0], None if dS is None else dS[1 + si])
        coef_t = got["c" + key]
        for row, nm in enumerate(("A", "D", "E")):
            within(stats, f"{name} {nm}", coef_t[row], c[nm], b[nm], ctx=f"{ctx} set {key}")
        ref_g = c["dgamma"] + (sk[0].to(F64) if sinks is not None else 0.0)
        ref_b = c["dbeta"] + (sk[1].to(F64) if sinks is not None else 0.0)
        within(stats, f"{name} dgamma", got["dg" + key], ref_g, b["dgamma"], ctx=f"{ctx} set {key}")
        within(stats, f"{name} dbeta", got["db" + key], ref_b, b["dbeta"], ctx=f"{ctx} set {key}")


def check_bwd_reduce(impl, C, rows, stats=None, kinds=MASK_KINDS, sets=(False, True), repeats=3):
    """bn_bwd_reduce, bn_bwd_coef (exact sums, grad_scale 0.25) and bn_bwd_reduce_coef (sinks
    given and absent, ``repeats`` calls in a row bit-equal)."""
    d = inputs(C, rows)
    count = float(rows)
    for kind in kinds:
        ms = mask_source(d, kind)
        for two in sets:
            ctx = f"(C={C}, rows={rows}, mask={kind}, two={two})"
            yb, mu_b, g_b, inv_b = (d["yb"], d["mu_b"], d["g_b"], d["inv_b"]) if two else (None,) * 4
            ref, abs_sums, _ = O.bwd_sums(d["dout"], ms, d["ya"], d["mu_a"], yb, mu_b)
            bound = reduce_bound(d, abs_sums)
            sums = impl.bwd_reduce(d["dout"], ms, d["ya"], d["mu_a"], yb, mu_b)
            within(stats, "bn_bwd_reduce", sums, ref, bound, ctx=ctx)
            for sinks in (None, d["sinks"]):
                sctx = f"{ctx} sinks={sinks is not None}"
                if kind == "act":   # the epilogue alone, on exact sums, with a gradient scale
                    got = impl.bwd_coef(ref, count, d["g_a"], d["mu_a"], d["inv_a"], g_b, mu_b, inv_b, sinks, 0.25)
                    _check_coef_result(stats, "bn_bwd_coef", got, d, ref, count, two, sinks, 0.25, None, sctx)
                two_step = impl.bwd_coef(sums, count, d["g_a"], d["mu_a"], d["inv_a"], g_b, mu_b, inv_b, sinks)
                for _ in range(repeats):
                    got = impl.bwd_reduce_coef(d["dout"], ms, d["ya"], d["mu_a"], yb, mu_b, count, d["g_a"],
                                               d["inv_a"], g_b, inv_b, sinks)
                    for k, v in two_step.items():
                        if v is not None:
                            same_bits(f"bn_bwd_reduce_coef {k} vs reduce + coef", got[k], v, sctx)
                _check_coef_result(stats, "bn_bwd_reduce_coef", got, d, ref, count, two, sinks, 1.0, bound, sctx)


def check_bwd_reduce3(impl, g, stats=None, repeats=3):
    """Two BN sets at a shape whose partial slab has g rows: the 3-set column reduction with the
    coefficient epilogue behind a multi-block combine."""
    C, rows = reduce3_case(g)
    check_bwd_reduce(impl, C, rows, stats, kinds=["act", "affine"] if g < 100 else ["act"], sets=(True,),
                     repeats=repeats)


def finalize_bounds(ref):
    b = dict(mean=U24 * ref["mean"].abs(), invstd=U24 * ref["invstd"].abs(), scale=2 * U24 * ref["scale"].abs(),
             shift=4 * U24 * ref["shift_terms"])
    if "running_mean" in ref:
        b.update(running_mean=4 * U24 * ref["rm_terms"], running_var=4 * U24 * ref["rv_terms"])
    return b


def check_finalize_result(stats, name, got, sums, count, gamma, beta, eps, mom, rm, rv, ctx=""):
    ref = O.finalize(sums, count, gamma, beta, eps, mom, rm, rv)
    for k, b in finalize_bounds(ref).items():
        within(stats, f"{name} {k}", got[k], ref[k], b, ctx=ctx)


def check_stats(impl, rows, C, stats=None, repeats=3):
    """bn_stats_reduce against the fp64 sum, bn_finalize on the same sums against the oracle,
    bn_stats_finalize bit-equal to the two (``repeats`` calls in a row)."""
    ctx = f"(rows={rows}, C={C})"
    slab = stat_slab(rows, C)
    g = _gen(rows, C, 23)
    gamma, beta, _ = channel_vectors(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    sums = impl.stats_reduce(slab)
    ref = slab.to(F64).sum(0)
    within(stats, "bn_stats_reduce", sums, ref, rows * U52 * slab.to(F64).abs().sum(0), ctx=ctx)
    count = float(rows * 16)
    fin = impl.finalize(sums, count, gamma, beta, EPS, MOMENTUM, rm, rv)
    check_finalize_result(stats, "bn_finalize", fin, sums, count, gamma, beta, EPS, MOMENTUM, rm, rv, ctx)
    for _ in range(repeats):
        one = impl.stats_finalize(slab, count, gamma, beta, EPS, MOMENTUM, rm, rv)
        for k, v in fin.items():
            same_bits(f"bn_stats_finalize {k} vs reduce + finalize", one[k], v, ctx)


def finalize_edge_cases():
    """(name, sums, count, gamma, beta, momentum, rm, rv) from the statistics of bf16 data."""
    C, rows = 40, 64
    g = _gen(C, rows, 31)
    y = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(BF16)
    y[:, 3] = 1.5                           # constant channels: Σy²/n − mean² is exactly 0 in fp64,
    y[:, 11] = -0.75                        # so these do NOT reach the var < 0 clamp
    s = O.stats(y)
    # the clamp: a conv epilogue hands Σy² over rounded to fp32; rounded down by one fp32 ulp,
    # the variance of the constant channels is −v²·2^-24 < 0 before the clamp. Unclamped, invstd
    # would be off by v²·2^-25 / eps (0.7 % and 0.2 %) and running_var negative at momentum 1.
    s_neg = s.clone()
    s_neg[1, [3, 11]] = s[1, [3, 11]] * (1.0 - U24)
    assert ((s_neg[1] / rows - (s_neg[0] / rows) ** 2)[[3, 11]] < -1e-8).all()
    gamma, beta, _ = channel_vectors(C, g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    n = float(rows)
    return [("constant channel", s, n, gamma, beta, MOMENTUM, rm, rv),
            ("negative variance clamped", s_neg, n, gamma, beta, 1.0, rm, rv),
            ("count 1", O.stats(y[:1]), 1.0, gamma, beta, MOMENTUM, rm, rv),
            ("no gamma", s, n, None, beta, MOMENTUM, rm, rv),
            ("no beta", s, n, gamma, None, MOMENTUM, rm, rv),
            ("no gamma, no beta", s, n, None, None, MOMENTUM, rm, rv),
            ("no update", s, n, gamma, beta, MOMENTUM, None, None),
            ("momentum 0", s, n, gamma, beta, 0.0, rm, rv),
            ("momentum 1", s, n, gamma, beta, 1.0, rm, rv),
            ("global count", s, 2 * n, gamma, beta, MOMENTUM, rm, rv)]


def check_finalize_edges(impl, stats=None):
    for name, s, n, gamma, beta, mom, rm, rv in finalize_edge_cases():
        got = impl.finalize(s, n, gamma, beta, EPS, mom, rm, rv)
        check_finalize_result(stats, "bn_finalize", got, s, n, gamma, beta, EPS, mom, rm, rv, f"({name})")
        if rm is None:
            assert "running_mean" not in got
        if name == "negative variance clamped":
            assert (got["running_var"][[3, 11]] == 0).all(), "var < 0 not clamped"
    # the zero variance and the guard, stated directly: invstd = 1 / sqrt(eps), one cast
    cases = finalize_edge_cases()
    expect = 1.0 / math.sqrt(float(np.float32(EPS)))
    for k in (0, 1):
        const = impl.finalize(cases[k][1], cases[k][2], None, None, EPS, MOMENTUM)["invstd"].to(F64)
        assert ((const[[3, 11]] - expect).abs() <= U24 * expect).all(), f"{cases[k][0]}: invstd != 1/sqrt(eps)"
    _, s, n, gamma, beta, mom, rm, rv = cases[2]
    one = impl.finalize(s, n, gamma, beta, EPS, mom, rm, rv)
    assert ((one["invstd"].to(F64) - expect).abs() <= U24 * expect).all(), "count 1: invstd != 1/sqrt(eps)"
    assert torch.isfinite(one["running_var"]).all(), "count 1: unbiased-variance guard"


def eval_inputs(C):
    g = _gen(C, 41)
    gamma, beta, rm = channel_vectors(C, g)
    rv = torch.rand(C, generator=g) + 0.1
    rv[0], rv[C // 2], rv[C - 1] = 1e-6, 1e4, 0.0
    return gamma, beta, rm, rv


def eval_affine_error(impl, C):
    """Largest relative error of scale (against |ref|) and of shift (against |β| + |mean·γ·invstd|)."""
    gamma, beta, rm, rv = eval_inputs(C)
    worst = 0.0
    for g_, b_ in ((gamma, beta), (None, None)):
        sc, sh = impl.eval_affine(g_, b_, rm, rv, EPS)
        rsc, rsh = O.eval_affine(g_, b_, rm, rv, EPS)
        terms = (b_.to(F64).abs() if b_ is not None else 0.0) + (rsh - (b_.to(F64) if b_ is not None else 0.0)).abs()
        worst = max(worst, ((sc.to(F64) - rsc).abs() / rsc.abs()).max().item(),
                    ((sh.to(F64) - rsh).abs() / terms).max().item())
    return worst


def check_eval_chain(impl, C, stats=None):
    """bn_eval_affine -> bn_apply: the bn_apply bound with the kernel's own scale and shift."""
    gamma, beta, rm, rv = eval_inputs(C)
    sc, sh = impl.eval_affine(gamma, beta, rm, rv, EPS)
    y = inputs(C, 5)["y"]
    out, _ = impl.apply(y, sc, sh, None, None, None, 0, False, False)
    z, T = O.apply(y, sc, sh, relu=False)
    within(stats, "bn_eval_affine -> bn_apply", out, z, U8 * z.abs() + U22 * T, ctx=f"(C={C})")


def small(cases):
    return [(C, rows) for C, rows in cases if rows <= SMALL_ROWS]


def run_small(impl, stats=None):
    """Every case of at most SMALL_ROWS rows through every comparison (the knob child)."""
    for C, rows in small(EW_CASES) + EW_KNOB_CASES:
        check_apply(impl, C, rows, stats)
        check_bwd_apply(impl, C, rows, stats)
    for C, rows in small(REDUCE_CASES):
        check_bwd_reduce(impl, C, rows, stats)
    for C in STATS_C:
        for rows in stats_rows_for(C):
            if rows <= SMALL_ROWS:
                check_stats(impl, rows, C, stats)
    check_finalize_edges(impl, stats)


KNOB_ENV = {"SDX_EW_BLOCKS": "8", "SDX_EW_BLOCKS_BWD": "16", "SDX_CR_GY": "4"}
CHILD_MARKER = "BN-KNOBS-OK"


def _child():
    import signal
    signal.alarm(240)       # the child's own limit: SIGALRM ends it
    assert all(os.environ.get(k) == v for k, v in KNOB_ENV.items()), "knobs not set"
    # the knobs move the cases onto other paths: several grid-stride iterations at 100 rows,
    # gy = 12 with empty trailing blocks at 9 rows
    assert ew_cap() == 8 and ew_cap(True) == 16
    assert ew_path(24, 3000) == (False, 4, 5) and ew_path(24, 3000, bwd=True) == (False, 2, 3)
    assert ew_path(64, 1000) == (True, 3, 4) and ew_path(64, 1000, bwd=True) == (True, 1, 2)
    assert col_reduce_gy(9) == 12 and col_reduce_per(9) == 1
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    stats = {}
    run_small(ExtImpl(m, torch.device("cuda:0")), stats)
    torch.cuda.synchronize()
    for k in sorted(stats):
        print(f"{k}: {stats[k]:.4f}")
    print(CHILD_MARKER)


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        _child()
