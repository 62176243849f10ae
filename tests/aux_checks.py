"""Cases, inputs, guards, fp32 twins and comparison functions of the max-pool, weight-prep and
probe-step oracle tests (oracle: tests/aux_oracle.py).

The comparison functions take an *implementation*: ``ExtImpl`` runs the HIP kernels
(csrc/kernels/pool.hip, wprep.hip, linear_ce.hip, linear_ce_sweep.hip) through the extension;
``TwinImpl`` runs CPU fp32 twins that follow each kernel's loops, optionally with a named
deliberate defect (``DEFECTS``). tests/test_aux_oracle.py holds the twins to the comparisons on
the CPU and shows that every defect fails its named case; tests/test_gpu_aux_oracle.py holds the
kernels to the same comparisons.

What is compared, and how.

  max-pool   y bit for bit except the sign of a zero (the comparison of the oracle is numeric;
             which zero comes back is tallied, not asserted); idx equal to the oracle's
             position. dy in integers and halves, |dy| <= 4: every sum is a multiple of 2^-1
             below 2^8 units (the guard), a bf16 value, so both backwards are bit-equal to the
             oracle and to each other. Random bf16 dy: the fp32 chain of n terms makes n − 1
             roundings of a partial sum of at most Σ|term| each, δ = (n − 1)·2^-24·Σ|term|, and
             the stored bf16 lies in [bf16(s − δ), bf16(s + δ)] (rounding is monotone).
  wprep      every 16-bit pattern of the whole output buffer: the slices against integer
             rne_bf16 of the source, the alignment gaps against the sentinel they were filled
             with.
  probe      exact regime: x, W integers in [−2, 2], b in halves: logits bit-equal, hits equal.
             SGD through linear_ce_sgd_raw with x, dz, buf integers, W in halves and lr, m, wd
             signed powers of two: every intermediate is a multiple of 2^-10 below 2^24 units
             (the guard), so W, b, both buffers and stats are bit-equal.
             Their softmax is far from the well-scaled one of the wide regime (|z| up to a few
             hundred), so dz and the row loss get a bound of their own there: the argument
             a = z − lse carries Δa <= u·(4·max|z| + 2·spread + 16) + γ(C) + 2^-19 (m, log s and
             their sum, the difference; the C exponentials of the sum s with their argument
             scaling u·|z − m| each and the sum's own roundings; log s <= ln 1024 to 1 ulp,
             times ln 2), exp(a) a relative Δa + 6u·|a| (its own argument scaling and ulp), and
             (e − onehot)·(1/B) another 2u / B. This is how a row with a bad label is shown to
             carry the plain softmax / B.
             wide regime (random fp32): loss, logits, dz by the rule of tests/test_gpu_ce_head.py
             (4 x fp32 torch's error on the same inputs + 2^-23·max|oracle|). One SGD step
             against the fp64 step from the same fp32 state and the same dz, u = 2^-24,
             γ(n) = n·u / (1 − n·u):
               g     fmaf chain over the B rows                e_g = γ(B)·Σ|dz·x|
               d     wd·w rounded, the sum rounded             e_d = e_g + u·|wd·w| + u·|d|
                     (a contracted fma makes one rounding, which is less)
               buf   one fmaf (none on the first step: buf = d) e_b = e_d + u·|buf|
               w     lr·buf rounded, the difference rounded    e_w = |lr|·e_b + u·|lr·buf| + u·|w|
             each bound times 1 + 2^-10 for the second-order terms left out. The bias has
             Σ|dz| in place of Σ|dz·x| (B − 1 plain additions).

No tolerance comes from a measurement.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import aux_oracle as O
from bn_checks import same_bits, within
from bnfold_checks import bf16_within, equal_at, fma32, r32
from conv_oracle import rne_bf16, trunc_bf16

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U24 = 2.0 ** -24
ULP = 2.0 ** -23
SLACK = 1.0 + 2.0 ** -10
GRID_CAP = 4096 * 256              # pool.hip grid_for: blocks x threads; beyond it the loop strides
SENT = -12352.0                    # a bf16 / fp32 value no case produces
SENT_BITS = 0x7FC1                 # a bf16 pattern rne_bf16 never returns for the inputs used


def gamma(n):
    return n * U24 / (1.0 - n * U24)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * p for k, p in zip(key, (1000003, 10007, 101, 13, 7))) % (2 ** 31))
    return g


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


class Guard:
    """Largest magnitude, in units, that a claimed-exact quantity reaches; asserted below limit."""

    def __init__(self):
        self.worst = {}

    def add(self, name, bound, unit, limit):
        v = float(bound.max() if isinstance(bound, torch.Tensor) else bound) / unit
        self.worst[name] = max(self.worst.get(name, 0.0), v)
        assert v < limit, f"exactness guard: {name} can reach {v:.4g} units: a wrong case, fix its inputs"

    @staticmethod
    def multiples(name, t, unit):
        q = t.to(F64) / unit
        assert torch.equal(q, q.round()), f"exactness guard: {name} is not a multiple of {unit}"


GUARD = Guard()


# =================================================================== max-pool =================

GEOMS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 3, 0), (3, 2, 0), (5, 2, 2), (1, 1, 0)]
SIZES = [(1, 1), (2, 5), (7, 7), (8, 8), (15, 17)]
_NC = [(1, 8), (3, 24), (1, 64), (3, 8), (1, 24), (3, 64)]


def _pool_cases():
    cases, i = {}, 0
    for k, s, p in GEOMS:
        for H, W in SIZES:
            if H + 2 * p < k or W + 2 * p < k:
                continue
            N, C = _NC[i % len(_NC)]
            i += 1
            cases[f"k{k}s{s}p{p} {H}x{W} N{N} C{C}"] = dict(k=k, s=s, p=p, N=N, H=H, W=W, C=C, neg_inf=False)
    # the windows (0, 0) and (0, 1) hold nothing but -inf and touch the padding
    cases["k3s2p1 7x7 N1 C8 -inf edge windows"] = dict(k=3, s=2, p=1, N=1, H=7, W=7, C=8, neg_inf=True)
    cases["k5s2p2 7x7 N3 C24 -inf edge windows"] = dict(k=5, s=2, p=2, N=3, H=7, W=7, C=24, neg_inf=True)
    return cases


POOL_CASES = _pool_cases()
NEG_INF_CASE = "k3s2p1 7x7 N1 C8 -inf edge windows"
UNCOVERED_CASE = "k3s3p0 8x8 N3 C8"
# the smallest work lists past the grid cap with a partial last trip: (k, s, p), x shape
POOL_GRID_FWD = dict(k=2, s=2, p=0, N=17, H=64, W=64, C=512)       # 17·32·32·64 = 1 114 112 groups
POOL_GRID_BWD = dict(k=3, s=2, p=1, N=17, H=32, W=32, C=512)       # 17·32·32·64 groups of dx
# (name, x shape, y shape or None, k, stride, pad): each must be refused by the bindings
POOL_REFUSED = [("stride 0", (1, 8, 8, 8), None, 3, 0, 1), ("stride -1", (1, 8, 8, 8), None, 3, -1, 1),
                ("k 0", (1, 8, 8, 8), None, 0, 1, 0), ("k -3", (1, 8, 8, 8), None, -3, 2, 0),
                ("y of another geometry", (1, 8, 8, 8), (1, 3, 3, 8), 3, 2, 1),
                ("y of another N", (2, 8, 8, 8), (1, 4, 4, 8), 3, 2, 1),
                ("y of another C", (1, 8, 8, 16), (1, 4, 4, 8), 3, 2, 1)]


def pool_inputs(name):
    """-> dict(x, dy_exact, dy_wide: fp32 tensors of bf16 values; geometry)"""
    def make():
        c = POOL_CASES[name]
        k, s, p, N, H, W, C = (c[n] for n in "kspNHWC")
        g = _gen(k, s, p, H * 100 + W, N * 100 + C)
        x = _ints(-3, 3, (N, H, W, C), g)
        x = torch.where((x == 0) & (torch.rand(x.shape, generator=g) < 0.5), -torch.zeros(()), x)
        if x.numel() >= 64:
            flat = x.reshape(-1)
            at = torch.randperm(flat.numel(), generator=g)[:6]
            flat[at[:3]] = float("inf")
            flat[at[3:]] = float("-inf")
        if c["neg_inf"]:
            x[0, 0:2, 0:4, :] = float("-inf")
        P, Q = O.out_size(H, k, s, p), O.out_size(W, k, s, p)
        dy_exact = _ints(-8, 8, (N, P, Q, C), g) / 2
        dy_wide = torch.randn(N, P, Q, C, generator=g).to(BF16).to(F32)
        return dict(c, x=x, P=P, Q=Q, dy_exact=dy_exact, dy_wide=dy_wide)
    return _cached(("pool", name), make)


def pool_grid_inputs(which):
    """The grid-stride case; the expected values come from torch's CPU max_pool2d (shown bit-equal
    to the tap-loop oracle, ties included, by tests/test_aux_oracle.py). Not cached: 140 MB."""
    c = POOL_GRID_FWD if which == "fwd" else POOL_GRID_BWD
    k, s, p, N, H, W, C = (c[n] for n in "kspNHWC")
    g = _gen(k, s, p, H, C)
    x = torch.randint(-3, 4, (N, H, W, C), generator=g, dtype=torch.int8).to(F32)
    P, Q = O.out_size(H, k, s, p), O.out_size(W, k, s, p)
    xt = x.permute(0, 3, 1, 2).requires_grad_(which == "bwd")
    y, at = F.max_pool2d(xt, k, s, p, return_indices=True)
    d = dict(c, x=x, P=P, Q=Q, y=y.detach().permute(0, 2, 3, 1).contiguous(),
             pos=torch_pos(at, W, k, s, p).permute(0, 2, 3, 1).contiguous())
    if which == "bwd":
        d["dy"] = torch.randint(-8, 9, (N, P, Q, C), generator=g, dtype=torch.int8).to(F32) / 2
        y.backward(d["dy"].permute(0, 3, 1, 2))
        d["dx"] = xt.grad.permute(0, 2, 3, 1).contiguous()
    d["x"] = x
    return d


def torch_pos(at, W, k, s, p):
    """torch's flat image offsets [N, C, P, Q] -> ddy·k + ddx of each window"""
    P, Q = at.shape[2], at.shape[3]
    h, w = at // W, at % W
    ddy = h - (torch.arange(P)[:, None] * s - p)
    ddx = w - (torch.arange(Q)[None, :] * s - p)
    return ddy * k + ddx


def guard_pool(d):
    _, pos = O.maxpool_fwd(d["x"], d["k"], d["s"], d["p"])
    _, mag, cnt = O.maxpool_bwd(pos, d["dy_exact"], d["H"], d["W"], d["k"], d["s"], d["p"])
    GUARD.multiples("pool dy", d["dy_exact"], 0.5)
    GUARD.add("pool Σ|dy|", mag, 0.5, 2.0 ** 8)
    assert int(cnt.max()) <= (-(-d["k"] // d["s"])) ** 2


def zero_tally(tally, x, y_got, k, s, p):
    """Among the windows whose maximum is 0 and that hold both +0 and -0: how often the result is +0."""
    pz = ((x == 0) & ~torch.signbit(x)).to(F64)
    nz = ((x == 0) & torch.signbit(x)).to(F64)
    both = (O.maxpool_fwd(pz, k, s, p)[0] > 0) & (O.maxpool_fwd(nz, k, s, p)[0] > 0) & (y_got == 0)
    first = O.maxpool_fwd(x, k, s, p)[0]
    tally["windows"] = tally.get("windows", 0) + int(both.sum())
    tally["+0"] = tally.get("+0", 0) + int((both & ~torch.signbit(y_got)).sum())
    tally["the first zero's sign"] = tally.get("the first zero's sign", 0) + \
        int((both & (torch.signbit(y_got) == torch.signbit(first))).sum())


def check_pool(impl, name, stats=None, tally=None):
    d = pool_inputs(name)
    k, s, p, H, W = d["k"], d["s"], d["p"], d["H"], d["W"]
    x = d["x"]
    y_ref, pos = O.maxpool_fwd(x, k, s, p)
    y0 = impl.pool_fwd(x, k, s, p)
    y1, idx = impl.pool_fwd_idx(x, k, s, p)
    same_bits("y of maxpool_fwd and of maxpool_fwd_idx", y0, y1, name)
    assert not torch.isnan(y1).any(), name
    assert torch.equal(y1.to(F64), y_ref), f"y differs from the oracle ({name})"      # -0 == +0
    if tally is not None:
        zero_tally(tally, x, y1, k, s, p)
    bad = idx.to(torch.int64) != pos
    assert not bad.any(), f"idx ({name}): {int(bad.sum())} differ, first at {bad.nonzero()[0].tolist()}: got " \
                          f"{int(idx[bad][0])}, oracle {int(pos[bad][0])}"
    # exact backward
    guard_pool(d)
    ref, _, cnt = O.maxpool_bwd(pos, d["dy_exact"], H, W, k, s, p)
    dx_r = impl.pool_bwd(x, y1, d["dy_exact"], k, s, p)
    dx_i = impl.pool_bwd_idx(idx, d["dy_exact"], H, W, k, s, p)
    equal_at("dx of maxpool_bwd_idx", dx_i.reshape(-1, d["C"]), rne_bf16(ref).reshape(-1, d["C"]), name)
    equal_at("dx of maxpool_bwd", dx_r.reshape(-1, d["C"]), rne_bf16(ref).reshape(-1, d["C"]), name)
    same_bits("dx of the two backwards", dx_r, dx_i, name)
    assert (dx_i[cnt == 0] == 0).all(), f"an input no window names got a gradient ({name})"
    # random dy: the bf16 interval
    ref, mag, cnt = O.maxpool_bwd(pos, d["dy_wide"], H, W, k, s, p)
    delta = (cnt - 1).clamp_min(0).to(F64) * U24 * mag
    bf16_within(stats, "pool dx (idx)", impl.pool_bwd_idx(idx, d["dy_wide"], H, W, k, s, p), ref, delta, name)
    bf16_within(stats, "pool dx (recompute)", impl.pool_bwd(x, y1, d["dy_wide"], k, s, p), ref, delta, name)


def check_pool_grid(impl, which):
    d = pool_grid_inputs(which)
    k, s, p = d["k"], d["s"], d["p"]
    groups = (d["N"] * d["P"] * d["Q"] if which == "fwd" else d["N"] * d["H"] * d["W"]) * d["C"] // 8
    assert groups > GRID_CAP and groups % GRID_CAP != 0, "the case must stride the grid, the last trip partial"
    y, idx = impl.pool_fwd_idx(d["x"], k, s, p)
    assert torch.equal(y, d["y"]), f"grid-stride {which}: y"
    assert torch.equal(idx.to(torch.int64), d["pos"]), f"grid-stride {which}: idx"
    if which == "fwd":
        assert torch.equal(impl.pool_fwd(d["x"], k, s, p), d["y"]), "grid-stride fwd: y without idx"
        return
    GUARD.add("pool grid-stride Σ|dy|", 9 * d["dy"].abs().max(), 0.5, 2.0 ** 8)
    assert torch.equal(impl.pool_bwd_idx(idx, d["dy"], d["H"], d["W"], k, s, p), d["dx"]), "grid-stride bwd_idx"
    assert torch.equal(impl.pool_bwd(d["x"], y, d["dy"], k, s, p), d["dx"]), "grid-stride bwd"


# ---- the fp32 twin of pool.hip (numpy float32; max and the exact sums need no rounding model) ----

def _np_tap(n_out, size, stride, pad, d):
    at = np.arange(n_out) * stride - pad + d
    return np.clip(at, 0, size - 1), (at >= 0) & (at < size)


def _drop_tail(out, wrong, fill):
    """grid_tail_dropped: the groups of the last, partial trip of the grid-stride loop stay unwritten."""
    if "grid_tail_dropped" in wrong:
        v = out.reshape(-1, 8)
        if v.shape[0] > GRID_CAP:
            v[v.shape[0] // GRID_CAP * GRID_CAP:] = fill
    return out


def twin_pool_fwd(x, k, s, p, wrong=()):
    N, H, W, C = x.shape
    P, Q = O.out_size(H, k, s, p), O.out_size(W, k, s, p)
    m = np.full((N, P, Q, C), -np.inf, np.float32)
    # at: the first in-image tap of the window (pool.hip), or tap 0 as before the fix
    p0 = np.maximum(0, p - np.arange(P) * s)[:, None]
    q0 = np.maximum(0, p - np.arange(Q) * s)[None, :]
    first = np.zeros((P, Q), np.int64) if "at_starts_at_0" in wrong else p0 * k + q0
    at = np.broadcast_to(first[None, :, :, None], m.shape).astype(np.uint8).copy()
    for ddy in range(k):
        hh, hv = _np_tap(P, H, s, p, ddy)
        for ddx in range(k):
            ww, wv = _np_tap(Q, W, s, p, ddx)
            v = x[:, hh][:, :, ww]
            inside = (hv[:, None] & wv[None, :])[None, :, :, None]
            if "pad_as_zero" in wrong:
                v = np.where(inside, v, np.float32(0))
                inside = np.ones_like(inside)
            take = inside & ((v >= m) if "last_max_wins" in wrong else (v > m))
            code = ddy * k + ddx
            if "pos_as_image_offset" in wrong:
                code = ((hh[:, None] * W + ww[None, :]) & 0xFF)[None, :, :, None]
            at = np.where(take, code, at).astype(np.uint8)
            m = np.where(take, v, m)
    return _drop_tail(m, wrong, SENT), _drop_tail(at, wrong, 255)


def _twin_gather(pos, dy, H, W, k, s, p, wrong):
    """The loops of both backward kernels: input pixel (h, w) visits its windows p outer, q inner."""
    N, P, Q, C = dy.shape
    h, w = np.arange(H), np.arange(W)
    p_lo, p_hi = np.maximum(0, (h + p - k + s) // s), np.minimum(P - 1, (h + p) // s)
    q_lo, q_hi = np.maximum(0, (w + p - k + s) // s), np.minimum(Q - 1, (w + p) // s)
    acc = np.zeros((N, H, W, C), np.float32)
    n = -(-k // s)
    for i in range(n):
        pp = p_lo + i
        pv = pp <= p_hi
        for j in range(n):
            qq = q_lo + j
            qv = qq <= q_hi
            if "bwd_drop_window" in wrong and i == n - 1 and j == n - 1 and n > 1:
                continue
            ppc, qqc = np.clip(pp, 0, P - 1), np.clip(qq, 0, Q - 1)
            code = ((h - (ppc * s - p))[:, None] * k + (w - (qqc * s - p))[None, :])[None, :, :, None]
            hit = (pv[:, None] & qv[None, :])[None, :, :, None] & (pos[:, ppc][:, :, qqc] == code)
            acc = (acc + np.where(hit, dy[:, ppc][:, :, qqc], np.float32(0))).astype(np.float32)
    t = torch.from_numpy(acc.astype(np.float64))
    out = (trunc_bf16(t) if "bwd_store_truncates" in wrong else rne_bf16(t)).numpy().astype(np.float32)
    return _drop_tail(out, wrong, SENT)


def twin_pool_bwd_idx(idx, dy, H, W, k, s, p, wrong=()):
    return _twin_gather(idx.astype(np.int64), dy, H, W, k, s, p, wrong)


def twin_pool_bwd(x, y, dy, k, s, p, wrong=()):
    """maxpool_bwd_kernel: the first in-image tap with v == y, recomputed per window."""
    N, H, W, C = x.shape
    P, Q = y.shape[1], y.shape[2]
    first = np.full(y.shape, -1, np.int64)
    for ddy in range(k):
        hh, hv = _np_tap(P, H, s, p, ddy)
        for ddx in range(k):
            ww, wv = _np_tap(Q, W, s, p, ddx)
            inside = (hv[:, None] & wv[None, :])[None, :, :, None]
            take = inside & (first < 0) & (x[:, hh][:, :, ww] == y)
            first = np.where(take, ddy * k + ddx, first)
    return _twin_gather(first, dy, H, W, k, s, p, wrong)


# =================================================================== weight prep ==============

# name -> (K, C, R, S, Cp or None, Linear)
WPREP_SHAPES = {
    "1x4 1x1": (1, 4, 1, 1, None, False),
    "10x12 3x3 scalar (K)": (10, 12, 3, 3, None, False),
    "68x20 3x3 vec ragged": (68, 20, 3, 3, None, False),
    "130x68 1x1 vec": (130, 68, 1, 1, None, False),
    "64x6 3x3 scalar, transposed": (64, 6, 3, 3, None, False),
    "16x3 7x7 stem Cp 8": (16, 3, 7, 7, 8, False),
    "5x3 3x3 stem Cp 8": (5, 3, 3, 3, 8, False),
    "128x100 1x1 vec": (128, 100, 1, 1, None, False),
    "linear 10x64 scalar (K)": (10, 64, 1, 1, None, True),
    "3x2 1x1 (leaves an alignment gap)": (3, 2, 1, 1, None, False),
}
_W = list(WPREP_SHAPES)
WPREP_TABLES = {
    "all, listed order": _W,
    "all, another order": [_W[i] for i in (7, 5, 0, 9, 8, 2, 6, 4, 1, 3)],
    "all, a padded stem last": [_W[i] for i in (8, 7, 6, 4, 9, 3, 2, 1, 0, 5)],
    **{f"alone: {n}": [n] for n in _W},
}
# fp32 patterns planted in every weight
WPREP_SPECIALS = [0x3F808000, 0x3F818000,                             # ties, kept bit even / odd
                  0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,     # one fp32 ulp either side
                  0xBF808000, 0xBF818000, 0xBF817FFF,
                  0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,     # round to inf / stay finite
                  0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80018000, 0x00400000,   # subnormals
                  0x00000000, 0x80000000, 0x7F800000, 0xFF800000]
UNPAD_CASES = [(1, 8, 3), (300, 8, 3), (7, 8, 8), (5, 1, 1)]


def wprep_table(name, dev="cpu"):
    """Toy modules through FlatParams and ConvWeightCache: the production segment table.
    -> dict(wc, convs, weights: the logical fp32 weights on the CPU)"""
    from simclr_pytorch_distributed_amd.ops.weights import ConvWeightCache
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    mods, pad = [], {}
    for n in WPREP_TABLES[name]:
        K, C, R, S, Cp, lin = WPREP_SHAPES[n]
        m = torch.nn.Linear(C, K, bias=False) if lin else \
            torch.nn.Conv2d(C, K, (R, S), bias=False).to(memory_format=torch.channels_last)
        if Cp:
            pad[id(m)] = Cp
        mods.append(m)
    model = torch.nn.ModuleList(mods).to(dev)
    flat = FlatParams(model)
    g = _gen(len(name), sum(map(ord, name)))
    master = torch.randn(flat.total, generator=g)
    spec = torch.from_numpy(np.array(WPREP_SPECIALS, dtype=np.uint32).view(np.float32).copy())
    for i, prm in enumerate(flat.params):
        n = prm.numel()
        for j, v in enumerate(spec):                       # (a small weight keeps the last ones)
            master[flat.offsets[i] + (7 * j + 3 * i) % n] = v
    with torch.no_grad():
        flat.flat.copy_(master)
    wc = ConvWeightCache(mods, flat.flat, pad)
    assert len(wc.seg_rows) == len(mods)
    return dict(name=name, wc=wc, convs=mods, flat=flat, weights=[m.weight.detach().cpu().clone() for m in mods])


def _bits(t64):
    """float64 holding bf16 values -> their 16-bit patterns (int64)"""
    return (t64.to(F32).contiguous().numpy().view(np.uint32) >> 16).astype(np.int64)


def check_wprep(impl, name, dev="cpu"):
    t = wprep_table(name, dev)
    wc = t["wc"]
    got = impl.wprep(t)                                   # int64 [len(buf)] of 16-bit patterns
    want = np.full(wc.buf.numel(), SENT_BITS, np.int64)
    owner = np.full(wc.buf.numel(), -1, np.int64)
    for i, (cv, w) in enumerate(zip(t["convs"], t["weights"])):
        e = wc.entries[id(cv)]
        fwd, tr = O.wprep_layouts(w, e["Cp"])
        assert (e["off_t"] >= 0) == (e["Cp"] == e["C"])
        for off, ref in ((e["off_k"], fwd), (e["off_t"], tr)):
            if off >= 0:
                assert (owner[off:off + ref.numel()] < 0).all(), "slices overlap"
                want[off:off + ref.numel()] = _bits(ref).reshape(-1)
                owner[off:off + ref.numel()] = 2 * i + (off == e["off_t"])
    bad = np.nonzero(got != want)[0]
    if len(bad):
        j = int(bad[0])
        where = "an alignment gap" if owner[j] < 0 else \
            f"the {'dgrad' if owner[j] % 2 else 'fwd'} slice of {WPREP_TABLES[name][owner[j] // 2]}"
        raise AssertionError(f"wprep ({name}): {len(bad)} patterns differ, first at {j} in {where}: got "
                             f"{got[j]:#06x}, want {want[j]:#06x}")
    return int((owner < 0).sum())


def twin_wprep(master, rows, tiles, n_out, wrong=()):
    """wprep_kernel block by block. master: float32 array; rows: ConvWeightCache.seg_rows."""
    out = np.full(n_out, SENT_BITS, np.int64)
    cvt = trunc_bf16 if "truncates" in wrong else rne_bf16

    def bf(a):
        return _bits(cvt(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))))

    segs = [dict(src=r[0], dst_k=r[1], dst_t=r[2], K=r[3] & 0xFFFFFFFF, RS=r[3] >> 32, C=r[4] & 0xFFFFFFFF,
                 Cp=r[4] >> 32, start=r[6]) for r in rows]
    for b in range(tiles):
        lo, hi = 0, len(segs) - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if (segs[mid]["start"] < b) if "seg_off_by_one" in wrong else (segs[mid]["start"] <= b):
                lo = mid
            else:
                hi = mid - 1
        s = segs[lo]
        K, RS, C, Cp = s["K"], s["RS"], s["C"], s["Cp"]
        kt, ct = (K + 63) // 64, (Cp + 63) // 64
        t = b - s["start"]
        if t < 0 or t >= kt * ct * RS:
            continue
        cti, t = t % ct, t // ct
        rs, kti = t % RS, t // RS
        k0, c0 = kti * 64, cti * 64
        if "k_tail_dropped" in wrong and k0 + 64 > K:
            continue
        vec = C % 4 == 0 and Cp == C and K % 4 == 0
        ks = np.arange(k0, min(K, k0 + 64))
        cs = np.arange(c0, min(Cp, c0 + 64))
        src = np.zeros((len(ks), len(cs)), np.float32)
        real = cs < C
        src[:, real] = master[s["src"] + (ks[:, None] * RS + rs) * C + cs[None, real]]
        tile = bf(src)
        wr = real if ("pad_not_zeroed" in wrong and not vec) else np.ones_like(real)
        out[s["dst_k"] + (ks[:, None] * RS + rs) * Cp + cs[None, wr]] = tile[:, wr]
        if s["dst_t"] < 0:
            continue
        cr = cs[real]
        if "t_indexed_kc" in wrong:
            out[s["dst_t"] + (ks[:, None] * RS + rs) * C + cr[None, :]] = tile[:, real]
        else:
            out[s["dst_t"] + (cr[None, :] * RS + rs) * K + ks[:, None]] = tile[:, real]
    return out


def unpad_inputs(rows, Cp, C):
    g = _gen(rows, Cp, C)
    src = _ints(-64, 64, (rows, Cp), g)
    dst = _ints(-64, 64, (rows, C), g)
    return src, torch.where(dst == 0, torch.ones(()), dst)


def check_unpad_add(impl, rows, Cp, C):
    src, dst = unpad_inputs(rows, Cp, C)
    once = O.unpad_add(src, dst)
    twice = O.unpad_add(src, once)
    GUARD.add("unpad_add", twice.abs().max(), 1.0, 2.0 ** 24)
    got1, got2, intact = impl.unpad_add(src, dst)
    equal_at("unpad_add", got1, once, f"({rows}, {Cp}, {C})")
    equal_at("unpad_add, second call", got2, twice, f"({rows}, {Cp}, {C})")
    assert intact, f"unpad_add wrote outside its sink ({rows}, {Cp}, {C})"


# =================================================================== probe step ===============

PROBE_K = [64, 128, 256, 1024, 2048]
PROBE_C = [1, 3, 5, 64, 65, 1000, 1024]
PROBE_B = [1, 4, 5, 37]
PROBE_WIDE_K = [128, 256, 1024]
PROBE_WIDE_CB = [(C, B) for C in (1, 3, 10, 70, 1000) for B in (1, 5, 37)]
# (C, K): C·K/4 below, at and above a multiple of 256
SGD_SHAPES = [(1, 64), (4, 256), (5, 64), (5, 256), (70, 512)]       # C·K/4 = 16, 256, 80, 320, 8960
SGD_CASES = [(C, K, B, first, wd) for C, K in SGD_SHAPES for B in (1, 37) for first in (0, 1) for wd in (0.0, 0.125)]
SGD_WIDE_LRS = [30.0, 0.5, 0.01]
SWEEP_CASE = dict(G=3, K=256, C=65, B=5)


def probe_inputs(K, C, B, seed=0):
    """Exact regime. Row 0 (C >= 2): the label ties the maximum. Row 1 (B >= 2, C >= 6): four classes
    above the label, one more level with it: it ties for 5th place. Rows 2, 3 (B >= 4): labels -1, C."""
    def make():
        g = _gen(K, C, B, seed)
        x = _ints(-2, 2, (B, K), g)
        W = _ints(-2, 2, (C, K), g)
        b = _ints(-4, 4, (C,), g) / 2
        y = torch.randint(0, C, (B,), generator=g)
        if C >= 2:
            x[0] = 0
            x[0, 0] = 1
            W[0:2, 0] = 2
            b[0:2] = 2
            y[0] = 0
        if B >= 2 and C >= 6:
            x[1] = 0
            x[1, 1] = 1
            W[:, 1] = -2
            W[0:4, 1] = 2
            b[0:4] = 2
            W[4:6, 1] = 1
            b[4:6] = 1
            y[1] = 4
        if B >= 4:
            y[2], y[3] = -1, C
        return x, W, b, y
    return _cached(("probe", K, C, B, seed), make)


def _rule(stats, name, got, t32, ref, ctx):
    """tests/test_gpu_ce_head.py: 4 x fp32 torch's error + 2^-23·max|oracle|; both errors printed."""
    e32 = float((t32.to(F64) - ref).abs().max())
    ek = float((got.to(F64) - ref).abs().max())
    allow = 4.0 * e32 + ULP * float(ref.abs().max())
    ratio = ek / allow if allow > 0 else (0.0 if ek == 0 else float("inf"))
    print(f"{ctx} {name}: kernel err {ek:.3e}, fp32 torch err {e32:.3e}, allowed {allow:.3e}, ratio {ratio:.3f}")
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), ratio)
    assert ek <= allow, f"{name} {ctx}: error {ek:.3e} > allowed {allow:.3e}"


def _torch32(x, W, b, y):
    """fp32 torch on the same inputs: logits, mean loss over the valid rows' sum / B, dz."""
    z = F.linear(x, W, b)
    C = W.shape[0]
    valid = (y >= 0) & (y < C)
    sm = torch.softmax(z, 1)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(len(y))[valid], y[valid]] = 1.0
    rows = torch.logsumexp(z, 1) - z.gather(1, y.clamp(0, C - 1)[:, None])[:, 0]
    return z, rows, (sm - onehot) / len(y)


def check_probe_fwd_exact(impl, K, C, B, stats=None):
    ctx = f"(K={K}, C={C}, B={B})"
    x, W, b, y = probe_inputs(K, C, B)
    GUARD.add("logits", (x.abs().to(F64) @ W.abs().to(F64).T + b.abs().to(F64)), 0.5, 2.0 ** 24)
    ref = O.classifier(x, W, b, y)
    got = impl.probe_fwd(x, W, b, y)
    equal_at("logits", got["z"], ref["z"], ctx)
    valid = ref["valid"]
    assert torch.equal(got["rowstat"][:, 1:].to(F64), ref["rowstat"][:, 1:]), f"hits per row {ctx}"
    assert torch.equal(torch.isnan(got["rowstat"][:, 0]), ~valid), f"row loss NaN exactly where the label is bad {ctx}"
    assert torch.equal(got["stats"][1:].to(F64), ref["stats"][1:]), f"hit counts {ctx}"
    assert bool(torch.isnan(got["stats"][0])) == bool((~valid).any()), f"stats[0] {ctx}"
    if C < 5:
        assert float(got["stats"][2]) == float(valid.sum()), f"C < 5: every valid row is a top-5 hit {ctx}"
    # the construction holds what it promises
    z, lab = ref["z"], y.clamp(0, C - 1)
    level = ((z == z.gather(1, lab[:, None])).sum(1) - 1)[valid]
    above = (z > z.gather(1, lab[:, None])).sum(1)[valid]
    if C >= 2:
        assert ((level > 0) & (above == 0)).any(), "no row whose label ties the maximum"
    if B >= 2 and C >= 6:
        assert ((level > 0) & (above == 4)).any(), "no row whose label ties for 5th place"
    # the softmax of these large integer logits, by the bound of the header
    zr = ref["z"]
    a = zr - torch.logsumexp(zr, 1, keepdim=True)
    zmax = zr.abs().max(1, keepdim=True).values
    spread = (zr.max(1, keepdim=True).values - zr.min(1, keepdim=True).values)
    e_arg = U24 * (4 * zmax + 2 * spread + 16) + gamma(C) + 2.0 ** -19
    within(stats, "exact-regime dz", got["dz"], ref["dz"], (a.exp() * (e_arg + 6 * U24 * a.abs()) + 2 * U24) / B, ctx=ctx)
    if valid.any():
        loss = ref["rowstat"][valid, 0]
        within(stats, "exact-regime row loss", got["rowstat"][valid, 0], loss,
               (e_arg[:, 0] + 2 * U24 * zmax[:, 0])[valid] + U24 * loss, ctx=ctx)


def check_probe_wide(impl, K, C, B, stats=None):
    from test_gpu_ce_head import _inputs
    ctx = f"(K={K}, C={C}, B={B})"
    x, W, b, y = _inputs(B, K, C, "cpu")
    ref = O.classifier(x, W, b, y)
    got = impl.probe_fwd(x, W, b, y)
    z32, rows32, dz32 = _torch32(x, W, b, y)
    _rule(stats, "logits", got["z"], z32, ref["z"], ctx)
    _rule(stats, "dz", got["dz"], dz32, ref["dz"], ctx)
    _rule(stats, "loss", got["loss"].reshape(1), rows32.mean().reshape(1), ref["rowstat"][:, 0].mean().reshape(1), ctx)
    assert torch.equal(got["stats"][1:].to(F64), ref["stats"][1:]), f"hit counts {ctx}"


def sgd_inputs(C, K, B, seed=0):
    def make():
        g = _gen(C, K, B, 5 + seed)
        return dict(x=_ints(-2, 2, (B, K), g), dz=_ints(-2, 2, (B, C), g), W=_ints(-4, 4, (C, K), g) / 2,
                    b=_ints(-4, 4, (C,), g) / 2, bufW=_ints(-3, 3, (C, K), g), bufb=_ints(-3, 3, (C,), g),
                    rowstat=torch.cat([_ints(0, 9, (B, 1), g), _ints(0, 1, (B, 2), g)], 1))
    return _cached(("sgd", C, K, B, seed), make)


def sgd_hyper(C, first, wd):
    """Signed powers of two; the signs vary with the case."""
    return dict(lr=-0.5 if C % 2 else 0.25, mom=-0.25 if first else 0.5, wd=wd)


def check_sgd_exact(impl, C, K, B, first, wd):
    ctx = f"(C={C}, K={K}, B={B}, first={first}, wd={wd})"
    d = sgd_inputs(C, K, B)
    h = sgd_hyper(C, first, wd)
    ref = O.sgd_step(d["x"], d["dz"], d["W"], d["b"], d["bufW"], d["bufb"], h["lr"], h["mom"], wd, first)
    unit = 2.0 ** -10
    for n in ("W", "b"):
        big = ref[f"g{n}_abs"] + abs(wd) * d[n].abs() + abs(h["mom"]) * d[f"buf{n}"].abs()
        GUARD.add(f"sgd {n}", big * max(1.0, abs(h["lr"])) + d[n].abs(), unit, 2.0 ** 24)
        for q in (ref[n], ref[f"buf{n}"], ref[f"g{n}"], wd * d[n].to(F64), h["lr"] * ref[f"buf{n}"]):
            GUARD.multiples(f"sgd {n}", q, unit)
    got = impl.sgd_raw(d, h["lr"], h["mom"], wd, first)
    for n in ("W", "bufW"):
        equal_at(n, got[n], ref[n], ctx)
    for n in ("b", "bufb"):
        equal_at(n, got[n], ref[n], ctx)
    equal_at("stats", got["stats"], d["rowstat"].to(F64).sum(0), ctx)
    assert got["intact"], f"the step wrote outside W, b and the buffers {ctx}"


def check_eval_untouched(impl, K, C, B):
    """The statistics-only call (linear_ce_step, train = False): logits and hits as the oracle's,
    the parameter views and the sentinels around them unchanged."""
    x, W, b, y = probe_inputs(K, C, B)
    ref = O.classifier(x, W, b, y)
    logits, stats, untouched = impl.probe_eval(x, W, b, y)
    equal_at("eval logits", logits, ref["z"])
    assert torch.equal(stats[1:].to(F64), ref["stats"][1:])
    assert untouched, "the statistics-only call changed a parameter or a sentinel"


def sgd_bounds(d, ref, lr, mom, wd, first, B):
    """The bounds of the header for one step from the fp32 state d -> dict(W, b, bufW, bufb)."""
    lr, mom, wd = O.f32_value(lr), O.f32_value(mom), O.f32_value(wd)
    out = {}
    for n in ("W", "b"):
        w, buf = d[n].to(F64), d[f"buf{n}"].to(F64)
        e_g = gamma(B) * ref[f"g{n}_abs"]
        dd = ref[f"g{n}"] + wd * w
        e_d = e_g + U24 * (wd * w).abs() + U24 * dd.abs()
        nb = ref[f"buf{n}"]
        e_b = e_d if first else e_d + U24 * nb.abs()
        e_w = abs(lr) * e_b + U24 * (lr * nb).abs() + U24 * ref[n].abs()
        out[f"buf{n}"] = SLACK * e_b + 1e-300
        out[n] = SLACK * e_w + 1e-300
    return out


def check_sgd_wide(impl, K, C, B, stats=None):
    """Three steps, lr 30 -> 0.01, each from the implementation's own fp32 state and its own dz."""
    from test_gpu_ce_head import _inputs
    x, W, b, y = _inputs(B, K, C, "cpu")
    d = dict(x=x, W=W, b=b, bufW=torch.zeros_like(W), bufb=torch.zeros_like(b))
    mom, wd = 0.9, 1e-3
    for step, lr in enumerate(SGD_WIDE_LRS):
        ctx = f"(K={K}, C={C}, B={B}, step {step}, lr {lr})"
        fw = impl.probe_fwd(d["x"], d["W"], d["b"], y)
        d["dz"], d["rowstat"] = fw["dz"], fw["rowstat"]
        first = int(step == 0)
        ref = O.sgd_step(x, d["dz"], d["W"], d["b"], d["bufW"], d["bufb"], lr, mom, wd, first)
        bound = sgd_bounds(d, ref, lr, mom, wd, first, B)
        got = impl.sgd_raw(d, lr, mom, wd, first)
        for n in ("W", "b", "bufW", "bufb"):
            within(stats, f"sgd {n}", got[n], ref[n], bound[n], ctx=ctx)
        assert got["intact"], ctx
        d.update({n: got[n] for n in ("W", "b", "bufW", "bufb")})


def check_sweep(impl, stats=None):
    c = SWEEP_CASE
    G, K, C, B = c["G"], c["K"], c["C"], c["B"]
    heads = [probe_inputs(K, C, B, seed=g) for g in range(G)]
    x, y = heads[0][0], heads[0][3]
    W = torch.stack([h[1] for h in heads]) / 2            # halves: heads differ, the products stay exact
    b = torch.stack([h[2] for h in heads])
    logits, st = impl.probe_sweep_eval(x, W, b, y)
    for g in range(G):
        ref = O.classifier(x, W[g], b[g], y)
        GUARD.add("sweep logits", x.abs().to(F64) @ W[g].abs().to(F64).T + b[g].abs().to(F64), 0.25, 2.0 ** 24)
        equal_at(f"sweep logits, head {g}", logits[g], ref["z"])
        assert torch.equal(st[g, 1:].to(F64), ref["stats"][1:]), f"sweep hits, head {g}"
        assert bool(torch.isnan(st[g, 0])) == bool((~ref["valid"]).any())


# ---- the fp32 twin of linear_ce.hip ----

def twin_probe_fwd(x, W, b, y, wrong=()):
    x, W, b = (t.numpy().astype(np.float32) for t in (x, W, b))
    B, C = x.shape[0], W.shape[0]
    bias = np.where(np.arange(C) < 4, b, np.float32(0)) if "bias_c_lt_4" in wrong else b
    z = ((x @ W.T).astype(np.float32) + bias).astype(np.float32)
    y = y.numpy()
    ok = (y >= 0) & (y < C)
    m = z.max(1, keepdims=True)
    lse = (m[:, 0] + np.log(np.exp(z - m, dtype=np.float32).sum(1, dtype=np.float32))).astype(np.float32)
    zl = np.where(ok, z[np.arange(B), np.clip(y, 0, C - 1)], np.float32(0))
    if "tie_is_miss" in wrong:
        above = (z >= zl[:, None]).sum(1) - ok
    else:
        above = (z > zl[:, None]).sum(1)
    onehot = np.zeros_like(z)
    onehot[np.arange(B)[ok], y[ok]] = 1
    dz = ((np.exp(z - lse[:, None], dtype=np.float32) - onehot) * np.float32(1.0 / B)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        rowstat = np.stack([np.where(ok, lse - zl, np.float32(np.nan)), (ok & (above < 1)).astype(np.float32),
                            (ok & (above < 5)).astype(np.float32)], 1).astype(np.float32)
    stats = rowstat.astype(np.float64).sum(0)
    t = torch.from_numpy
    return dict(z=t(z), dz=t(dz), rowstat=t(rowstat), stats=t(stats).to(F32), loss=torch.tensor(float(np.float32(stats[0] / B))))


def twin_sgd(d, lr, mom, wd, first, wrong=()):
    """linear_ce_sgd_kernel: the fmaf chain over the rows, then the update, rounding by rounding."""
    x, dz = d["x"].to(F64).numpy(), d["dz"].to(F64).numpy()
    lr, mom, wd = (O.f32_value(v) for v in (lr, mom, wd))
    B = x.shape[0]
    out = {}
    for n in ("W", "b"):
        w, buf = d[n].to(F64).numpy(), d[f"buf{n}"].to(F64).numpy()
        g = np.zeros_like(w)
        for r in range(B):
            g = fma32(dz[r][:, None], x[r][None, :], g) if n == "W" else r32(g + dz[r])
        decay = 0.0 if (n == "b" and "bias_no_wd" in wrong) or "wd_after_momentum" in wrong else wd
        dd = r32(g + r32(decay * w))
        nb = dd if (first and "momentum_when_first" not in wrong) else fma32(mom, buf, dd)
        step = r32(nb + r32(wd * w)) if "wd_after_momentum" in wrong else nb
        out[n] = torch.from_numpy(r32(w - r32(lr * step))).to(F32)
        out[f"buf{n}"] = torch.from_numpy(nb).to(F32)
    out["stats"] = torch.from_numpy(r32(d["rowstat"].to(F64).numpy().sum(0))).to(F32)
    out["intact"] = True
    return out


DEFECTS = ["pad_as_zero", "last_max_wins", "pos_as_image_offset", "at_starts_at_0", "bwd_drop_window",
           "grid_tail_dropped", "bwd_store_truncates",
           "t_indexed_kc", "pad_not_zeroed", "k_tail_dropped", "truncates", "seg_off_by_one",
           "tie_is_miss", "bias_c_lt_4", "momentum_when_first", "wd_after_momentum", "bias_no_wd"]


# =================================================================== implementations ==========

class TwinImpl:
    def __init__(self, wrong=()):
        self.wrong = set(wrong)
        assert self.wrong <= set(DEFECTS), self.wrong

    @staticmethod
    def _n(t):
        return t.numpy().astype(np.float32)

    def pool_fwd(self, x, k, s, p):
        return torch.from_numpy(twin_pool_fwd(self._n(x), k, s, p, self.wrong)[0])

    def pool_fwd_idx(self, x, k, s, p):
        y, at = twin_pool_fwd(self._n(x), k, s, p, self.wrong)
        return torch.from_numpy(y), torch.from_numpy(at)

    def pool_bwd(self, x, y, dy, k, s, p):
        return torch.from_numpy(twin_pool_bwd(self._n(x), self._n(y), self._n(dy), k, s, p, self.wrong))

    def pool_bwd_idx(self, idx, dy, H, W, k, s, p):
        return torch.from_numpy(twin_pool_bwd_idx(idx.numpy(), self._n(dy), H, W, k, s, p, self.wrong))

    def wprep(self, t):
        wc = t["wc"]
        return twin_wprep(wc.master.cpu().numpy(), wc.seg_rows, wc.tiles, wc.buf.numel(), self.wrong)

    def unpad_add(self, src, dst):
        once = (dst.numpy() + src.numpy()[:, :dst.shape[1]]).astype(np.float32)
        twice = (once + src.numpy()[:, :dst.shape[1]]).astype(np.float32)
        return torch.from_numpy(once), torch.from_numpy(twice), True

    def probe_fwd(self, x, W, b, y):
        return twin_probe_fwd(x, W, b, y, self.wrong)

    def sgd_raw(self, d, lr, mom, wd, first):
        return twin_sgd(d, lr, mom, wd, first, self.wrong)

    def probe_eval(self, x, W, b, y):
        r = twin_probe_fwd(x, W, b, y, self.wrong)
        return r["z"], r["stats"], True

    def probe_sweep_eval(self, x, W, b, y):
        r = [twin_probe_fwd(x, W[g], b[g], y, self.wrong) for g in range(W.shape[0])]
        return torch.stack([q["z"] for q in r]), torch.stack([q["stats"] for q in r])


class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""
    PAD = 8

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _bf(self, t):
        return t.to(BF16).contiguous().to(self.dev)

    def pool_fwd(self, x, k, s, p):
        return self.m.maxpool_fwd(self._bf(x), k, s, p).cpu().to(F32)

    def pool_fwd_idx(self, x, k, s, p):
        y, idx = self.m.maxpool_fwd_idx(self._bf(x), k, s, p)
        return y.cpu().to(F32), idx.cpu()

    def pool_bwd(self, x, y, dy, k, s, p):
        return self.m.maxpool_bwd(self._bf(x), self._bf(y), self._bf(dy), k, s, p).cpu().to(F32)

    def pool_bwd_idx(self, idx, dy, H, W, k, s, p):
        return self.m.maxpool_bwd_idx(idx.to(self.dev), self._bf(dy), H, W, k, s, p).cpu().to(F32)

    def wprep(self, t):
        wc = t["wc"]
        assert wc.native, "the weight cache did not take the native path"
        wc.buf.view(torch.int16).fill_(SENT_BITS)
        wc.refresh()
        torch.cuda.synchronize()
        return wc.buf.view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF

    def _views(self, shapes):
        """Contiguous views of the given shapes inside one sentinel buffer, PAD sentinels around each
        (sizes rounded up to 4 elements: every view starts 16-byte aligned)."""
        offs, n = [], self.PAD
        for sh in shapes:
            offs.append(n)
            n += -(-int(np.prod(sh)) // 4) * 4 + self.PAD
        buf = torch.full((n,), SENT, device=self.dev)
        views = [buf[o:o + int(np.prod(sh))].view(sh) for o, sh in zip(offs, shapes)]
        outside = torch.ones(n, dtype=torch.bool)
        for o, sh in zip(offs, shapes):
            outside[o:o + int(np.prod(sh))] = False
        return buf, views, outside

    def unpad_add(self, src, dst):
        buf, (sink,), outside = self._views([tuple(dst.shape)])
        sink.copy_(dst)
        s = src.to(self.dev)
        self.m.unpad_add(s, sink)
        once = sink.cpu().clone()
        self.m.unpad_add(s, sink)
        host = buf.cpu()
        return once, sink.cpu().clone(), bool((host[outside] == SENT).all())

    def probe_fwd(self, x, W, b, y):
        z, dz, rowstat, stats, loss = self.m.ce_head_fwd(*(t.to(self.dev) for t in (x, W, b, y)), True)
        return dict(z=z.cpu(), dz=dz.cpu(), rowstat=rowstat.cpu(), stats=stats.cpu(), loss=loss.cpu())

    def sgd_raw(self, d, lr, mom, wd, first):
        names = ("W", "bufW", "b", "bufb")
        buf, views, outside = self._views([tuple(d[n].shape) for n in names])
        for v, n in zip(views, names):
            v.copy_(d[n])
        W, bufW, b, bufb = views
        stats = self.m.linear_ce_sgd_raw(d["x"].to(self.dev), d["dz"].to(self.dev), W, b, bufW, bufb, lr, mom, wd,
                                         bool(first), d["rowstat"].to(self.dev))
        host = buf.cpu()
        out = {n: v.cpu().clone() for v, n in zip(views, names)}
        out["stats"] = stats.cpu()
        out["intact"] = bool((host[outside] == SENT).all())
        return out

    def probe_eval(self, x, W, b, y):
        buf, (Wv, bv), _ = self._views([tuple(W.shape), tuple(b.shape)])
        Wv.copy_(W)
        bv.copy_(b)
        before = buf.clone()
        logits, stats = self.m.linear_ce_step(x.to(self.dev), Wv, bv, y.to(self.dev), None, None, 0.5, 0.5, 0.125,
                                              False, False)
        torch.cuda.synchronize()
        return logits.cpu(), stats.cpu(), bool(torch.equal(buf, before))

    def probe_sweep_eval(self, x, W, b, y):
        G = W.shape[0]
        logits, st = self.m.linear_ce_sweep_step(x.to(self.dev), W.contiguous().to(self.dev), b.contiguous().to(self.dev),
                                                 y.to(self.dev), None, None, [0.1] * G, 0.9, [0.0] * G, False, False)
        return logits.cpu(), st.cpu()


# name -> the comparison that must fail with that defect
DEFECT_CASES = {
    "pad_as_zero": lambda i: check_pool(i, "k3s2p1 7x7 N1 C64"),
    "last_max_wins": lambda i: check_pool(i, "k3s2p1 7x7 N1 C64"),
    "pos_as_image_offset": lambda i: check_pool(i, "k3s1p1 7x7 N3 C64"),
    "at_starts_at_0": lambda i: check_pool(i, NEG_INF_CASE),
    "bwd_drop_window": lambda i: check_pool(i, "k3s1p1 7x7 N3 C64"),
    "grid_tail_dropped": lambda i: check_pool_grid(i, "fwd"),
    "bwd_store_truncates": lambda i: check_pool(i, "k3s1p1 7x7 N3 C64"),
    "t_indexed_kc": lambda i: check_wprep(i, "alone: 64x6 3x3 scalar, transposed"),
    "pad_not_zeroed": lambda i: check_wprep(i, "alone: 5x3 3x3 stem Cp 8"),
    "k_tail_dropped": lambda i: check_wprep(i, "alone: 68x20 3x3 vec ragged"),
    "truncates": lambda i: check_wprep(i, "alone: 10x12 3x3 scalar (K)"),
    "seg_off_by_one": lambda i: check_wprep(i, "all, listed order"),
    "tie_is_miss": lambda i: check_probe_fwd_exact(i, 64, 64, 4),
    "bias_c_lt_4": lambda i: check_probe_fwd_exact(i, 128, 5, 5),
    "momentum_when_first": lambda i: check_sgd_exact(i, 5, 64, 37, 1, 0.0),
    "wd_after_momentum": lambda i: check_sgd_exact(i, 4, 256, 1, 0, 0.125),
    "bias_no_wd": lambda i: check_sgd_exact(i, 70, 512, 37, 0, 0.125),
}
