"""Cases, inputs, bounds, the fp32 twin and the comparison functions of the BN3 fold oracle tests.

The comparison functions take an *implementation*: ``ExtImpl`` runs the HIP kernels of
csrc/kernels/bnfold.hip through the test-only bindings (bnfold_prep, bnfold_colsum, bnfold_wgrad,
bnfold_rowdot); ``TwinImpl`` runs a CPU fp32 twin that follows each kernel's summation order,
optionally with a named deliberate defect (``DEFECTS``). tests/test_bnfold_oracle.py holds the
twin to the comparisons on the CPU and shows that every defect is caught at its named case;
tests/test_gpu_bnfold_oracle.py holds the kernels to the same comparisons.

Two regimes.

  exact  W3 in {−2..2}; A, D powers of two (with sign), E, a2, G, S, cs small integers, μ and
         the sinks dyadic, rows = 64. Every fp32 product and partial sum is then an integer
         multiple of a power of two (the unit) below 2^24 units — the guard asserts it — so a
         fp32 value is the real number whatever the order or the contraction, and Wd, Mx, b,
         the column sums (per block too), dW3 and both rowdot rows are compared bit for bit.
         The case "corr" has A = 1 + 2^-10 (A·W3 is not a bf16 value), |Mx| > 256 (Mx is not a
         bf16 value either) and μ such that mean(dz) = −(E + D·μ)/A is a small integer: both
         correction terms of b are non-zero and still exact.
  wide   random fp32 / bf16 inputs, rows = 1000. Bounds, with u = 2^-24, γ(n) = n·u / (1 − n·u)
         (n fp32 roundings, each of a partial sum of at most Σ|term|):

  Wd     bit-equal: one fp32 product, one nearest-even rounding.
  Mx     δ = γ(ceil(C/P) + P + 10)·Σ_c|W·D·W|: the fmaf chain of one lane group, the P − 1
         additions of the groups, the rounding of W·D; the stored bf16 lies in
         [bf16(ref − δ), bf16(ref + δ)] (rounding is monotone).
  b      against the weights actually stored (bnfold_oracle.prep_bias):
         γ(2·ceil(C/1024) + 10 + K/KW + 10 + 8)·Σ|term|    both fmaf per trip, the two LDS trees,
                                                            the k0 trips, mean(dz) (product, sum,
                                                            quotient), cs/rows (reciprocal,
                                                            product), the last addition
         + u·Σ_c|mean(dz)·A·W|                              A·W rounded before Wd is subtracted
         + Σ_k|mean(a2)[k]|·δ_Mx[l][k]                      the kernel's own Mx before rounding
  colsum partial γ(trips + 256/(K/8))·Σ|x| of the block; cs γ(trips + 256/(K/8) + 32 + 16)·Σ|x|:
         a thread's chunks, the LDS column of its channel group, then 512 / 16 partials per lane
         group and the 16 groups.
  wgrad  γ(K + ncs + 4)·Σ|term| (the W·S chain, the cs partials, three products, two sums,
         the sink); the three-term sum may or may not be contracted, so nothing is bit-exact.
  rowdot |double(hi) + double(lo) − ref| <= K·2^-53·Σ|term| + 2^-48·|ref|, |lo| <= ulp(hi)/2.

No tolerance comes from a measurement.
"""
from __future__ import annotations

import numpy as np
import torch

import bnfold_oracle as O
from bn_checks import same_bits, within
from conv_oracle import rne_bf16

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U24, U53, U48 = 2.0 ** -24, 2.0 ** -53, 2.0 ** -48
LIMIT = 2.0 ** 24
REGIMES = ("exact", "wide")
SENT = -12352.0                    # a bf16 value no case produces: untouched padding keeps it
PAD = 64

# ---------------------------------------------------------------- mirrors of the launchers ----
PREP_NT = 1024
COLSUM_BLOCKS, COLSUM_NT = 512, 256
COLSUM_STRIDE = COLSUM_BLOCKS * COLSUM_NT


def prep_path(C, K):
    """launch_bnfold_prep / bnfold_prep_kernel: k lanes per group, lane groups, k0 trips, Wd
    blocks, whether a Wd thread takes a second grid-stride element, trips of the b loop."""
    KW = PREP_NT if K >= PREP_NT else K
    n = K * C
    gw = min(256, -(-n // PREP_NT))
    return dict(KW=KW, P=PREP_NT // KW, k0_trips=K // KW, gw=gw, wd_strided=n > gw * PREP_NT,
                c_trips=-(-C // PREP_NT))


def prep_accepts(C, K, ldw=0, ldm=0):
    ldw, ldm = ldw or C, ldm or K
    if ldw < C or ldm < K:
        return False
    return 0 < C <= 8192 and K > 0 and (PREP_NT % K if K < PREP_NT else K % PREP_NT) == 0


def colsum_accepts(K):
    return K > 0 and K % 8 == 0 and K <= 2048 and 256 % (K // 8) == 0


def colsum_trips(n8):
    """(fewest, most) trips of the 4-way unrolled loop and of its tail over all threads."""
    e0 = np.arange(COLSUM_STRIDE)
    n_e = np.where(e0 < n8, -(-(n8 - e0) // COLSUM_STRIDE), 0)
    return (int((n_e // 4).min()), int((n_e // 4).max())), (int((n_e % 4).min()), int((n_e % 4).max()))


def wgrad_block(K):
    return (K + 63) // 64 * 64 if K < 256 else 256


def gamma(n):
    return n * U24 / (1.0 - n * U24)


def mx_depth(C, K):
    p = prep_path(C, K)
    return -(-C // p["P"]) + p["P"] + 10


def bias_depth(C, K):
    p = prep_path(C, K)
    return 2 * p["c_trips"] + 10 + p["k0_trips"] + 10 + 8


def colsum_depths(K, rows):
    trips = -(-(rows * K // 8) // COLSUM_STRIDE)
    part = trips + COLSUM_NT // (K // 8)
    return part, part + COLSUM_BLOCKS // 16 + 16


# ---------------------------------------------------------------- case tables -----------------

def _p(C, K, mu=True, cs=True, rows=True, cat=False, a0=False, corr=False):
    return dict(C=C, K=K, mu=mu, cs=cs, rows=rows, cat=cat, a0=a0, corr=corr)


PREP_CASES = {
    "P > C (1, 8)": _p(1, 8),
    "(7, 64) cat": _p(7, 64, cat=True),
    "(7, 64) separate": _p(7, 64),
    "(7, 64) no mu": _p(7, 64, mu=False),
    "(7, 64) no cs": _p(7, 64, cs=False, cat=True),
    "(7, 64) neither": _p(7, 64, mu=False, cs=False),
    "(7, 64) rows 0": _p(7, 64, rows=False, cat=True),
    "(7, 64) A = 0": _p(7, 64, a0=True),
    "production (256, 64)": _p(256, 64, cat=True),
    "production (256, 64) A = 0": _p(256, 64, cat=True, a0=True),
    "production (512, 128)": _p(512, 128, cat=True),
    "corr (256, 64)": _p(256, 64, cat=True, corr=True),
    "C > 1024, Wd grid-stride (1030, 512)": _p(1030, 512),
    "P = 1 (64, 1024)": _p(64, 1024, cat=True),
    "two k0 trips (64, 2048)": _p(64, 2048),
    "largest C (8192, 8)": _p(8192, 8, cat=True),
}
PREP_REFUSED = {"K = 96": (64, 96, 0, 0), "K = 1536": (64, 1536, 0, 0), "C = 8193": (8193, 8, 0, 0),
                "ldw < C": (64, 64, 63, 0), "ldm < K": (64, 64, 0, 63)}

_S = COLSUM_STRIDE
COLSUM_N8 = [1, 255, _S - 1, _S + 3, 4 * _S + _S + 77]
# (K, rows): every n8 = rows·K/8 of the list at K = 8; the wider K at the nearest row count above
COLSUM_CASES = [(8, n8) for n8 in COLSUM_N8] + \
               [(K, -(-n8 // (K // 8))) for K, n8 in ((64, 255), (64, _S + 3), (128, 1), (128, 5 * _S + 77),
                                                     (2048, _S - 1), (2048, 5 * _S + 77))]
COLSUM_REFUSED = [12, 24, 4096]

# (C, K, ncs, accumulate)
WGRAD_CASES = [(1, 8, 1, 0), (1, 8, 3, 1), (5, 72, 3, 0), (5, 72, 512, 1), (256, 64, 1, 1), (256, 64, 3, 0),
               (3, 320, 512, 0), (3, 320, 1, 1), (2, 8192, 3, 1)]
# (C, K, ns)
ROWDOT_CASES = [(1, 8, 2), (1, 8, 3), (7, 100, 2), (7, 100, 3), (512, 128, 2), (512, 128, 3)]
ROWDOT_KINDS = ("exact", "wide", "cancel")
ROWDOT_REFUSED = [1, 4]


# ---------------------------------------------------------------- inputs ----------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * p for k, p in zip(key, (1000003, 10007, 101, 13))) % (2 ** 31))
    return g


def _choice(values, n, g):
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), (n,), generator=g)]


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def _signed(n, g):
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (sign * (torch.rand(n, generator=g) + 0.5)).to(F32)


def coef_exact(C, g, positive_d=False):
    A = _choice([1.0, 2.0, -1.0, 0.5, -2.0, 4.0], C, g)
    D = _choice([1.0, 2.0, 0.5] if positive_d else [1.0, -1.0, 0.5, 2.0, -0.5], C, g)
    return A, D, _ints(-3, 3, (C,), g)


def coef_wide(C, g):
    return _signed(C, g), _signed(C, g) * 0.25, torch.randn(C, generator=g)


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def prep_inputs(name, regime):
    """-> dict(coef [3C], W [C][K] (bf16 values in fp32), mu | None, cs | None, rows, unit)"""
    def make():
        p = PREP_CASES[name]
        C, K = p["C"], p["K"]
        g = _gen(C, K, len(name), regime == "wide")
        rows = 0
        if regime == "exact":
            W = _ints(-2, 2, (C, K), g)
            A, D, E = coef_exact(C, g, positive_d=p["corr"])
            if p["corr"]:
                A = torch.full((C,), 1.0 + 2.0 ** -10)
                j = _ints(-3, 3, (C,), g)                    # the mean(dz) the kernel must find
                mu = ((-j.double() * A.double() - E.double()) / D.double()).to(F32)
                assert torch.equal(mu.double() * D.double() + E.double(), -j.double() * A.double())
            else:
                mu = _ints(-8, 8, (C,), g) / 4
            cs = _ints(-64, 64, (K,), g)
            if p["rows"]:
                rows = 64
        else:
            W = torch.randn(C, K, generator=g).to(BF16).to(F32)
            A, D, E = coef_wide(C, g)
            mu = torch.randn(C, generator=g)
            if p["rows"]:
                rows = 1000
            cs = (torch.rand(K, generator=g) * 1000).to(F32)
        if p["a0"]:
            A[C // 2] = 0.0
            A[0] = 0.0
        return dict(C=C, K=K, cat=p["cat"], coef=torch.cat([A, D, E]).contiguous(), W=W, mu=mu if p["mu"] else None,
                    cs=cs if p["cs"] else None, rows=rows, unit=2.0 ** -10 if p["corr"] else 2.0 ** -7)
    return _cached(("prep", name, regime), make)


def colsum_inputs(K, rows, regime):
    def make():
        g = _gen(K, rows, 7, regime == "wide")
        if regime == "exact":
            return _ints(-8, 8, (rows, K), g)
        return (torch.randn(rows, K, generator=g) + 0.5).to(BF16).to(F32)
    return _cached(("colsum", K, rows, regime), make)


def wgrad_inputs(C, K, ncs, regime):
    def make():
        g = _gen(C, K, ncs, regime == "wide")
        if regime == "exact":
            A, D, E = coef_exact(C, g)
            W = _ints(-2, 2, (C, K), g)
            G = _ints(-64, 64, (C, K), g)
            S = torch.randint(-8, 9, (K, K), generator=g, dtype=torch.int8).to(F32)
            cs = _ints(-8, 8, (ncs, K), g)
            sink = _ints(-256, 256, (C, K), g) / 2
        else:
            A, D, E = coef_wide(C, g)
            W = torch.randn(C, K, generator=g).to(BF16).to(F32)
            G = torch.randn(C, K, generator=g) * 8
            S = torch.randn(K, K, generator=g)
            cs = torch.randn(ncs, K, generator=g) * 4
            sink = torch.randn(C, K, generator=g) * 4
        assert K == 1 or not torch.equal(S, S.T)
        return dict(C=C, K=K, coef=torch.cat([A, D, E]).contiguous(), W=W, G=G, S=S, cs=cs, sink=sink)
    if K >= 4096:      # a 256 MB S: made again for each use, not kept
        return make()
    return _cached(("wgrad", C, K, ncs, regime), make)


def rowdot_inputs(C, K, kind):
    def make():
        g = _gen(C, K, ROWDOT_KINDS.index(kind), 3)
        if kind == "exact":
            # even integers, 2·2^23 and one odd 2^23 + 1: the fp64 sum is exact, odd and above
            # 2^24, where fp32 holds even integers only, so lo is ±1 in every row
            W = _ints(-2, 2, (C, K), g)
            G = 2 * _ints(-2 ** 18, 2 ** 18, (C, K), g)
            W[:, 0], G[:, 0] = 2.0, 2.0 ** 23
            W[:, 1], G[:, 1] = 1.0, 2.0 ** 23 + 1
            return W, G
        W = torch.randn(C, K, generator=g).to(BF16).to(F32)
        W = torch.where(W == 0, torch.ones(()), W)
        G = torch.randn(C, K, generator=g) * 8
        if kind == "cancel" and K > 1:
            # the last product cancels the rest up to one fp32 rounding: |ref| << Σ|term|
            rest = (W[:, :-1].double() * G[:, :-1].double()).sum(1)
            G[:, -1] = (-rest / W[:, -1].double()).to(F32)
        return W, G
    return _cached(("rowdot", C, K, kind), make)


# ---------------------------------------------------------------- the exactness guard ---------

class Guard:
    """Per claimed-exact quantity, the largest magnitude a partial sum can reach (Σ|term|) in
    units of the terms' common power of two; every one must stay below 2^24 (2^53: rowdot)."""

    def __init__(self):
        self.worst = {}

    def add(self, name, bound, unit=1.0, limit=LIMIT):
        v = float(bound.max() if isinstance(bound, torch.Tensor) else bound) / unit
        self.worst[name] = max(self.worst.get(name, 0.0), v)
        assert v < limit, f"exactness guard: {name} can reach {v:.4g} units: a wrong case, fix its inputs"

    @staticmethod
    def multiples(name, t, unit):
        q = t.to(F64) / unit
        assert torch.equal(q, q.round()), f"exactness guard: {name} is not a multiple of {unit}"


GUARD = Guard()


def guard_prep(d):
    """The exact-regime claim for one prep case; -> Σ|term| of Mx and of b."""
    C, K, unit = d["C"], d["K"], d["unit"]
    A, D, E = O.split_coef(d["coef"], C)
    W = d["W"].to(F64)
    mx, mx_abs = O.prep_mx(d["coef"], W)
    GUARD.multiples("Mx", mx, 0.5)
    GUARD.add("Mx", mx_abs, 0.5)
    wd = O.prep_wd(d["coef"], W)
    pb = O.prep_bias(d["coef"], W, d["mu"], d["cs"], d["rows"], wd, rne_bf16(mx))
    ex = A[:, None] * W
    assert torch.equal(O.f32(ex), ex), "exactness guard: A·W is not a fp32 value"
    if d["mu"] is not None:
        nz = A != 0
        m1 = pb["m1"]
        # the kernel's quotient is exact where the correction is not 0: E + D·μ and m1 are fp32 values
        live = nz & ((ex - wd.T).abs().sum(1) > 0)
        s = E + D * d["mu"].to(F64)
        assert torch.equal(O.f32(s), s) and torch.equal(O.f32(m1[live]), m1[live])
        GUARD.multiples("mean(dz) where it counts", m1[live], 1.0)
    if d["cs"] is not None and d["rows"]:
        assert d["rows"] & (d["rows"] - 1) == 0, "exact regime: rows must be a power of two"
    GUARD.multiples("b", pb["b"], unit)
    GUARD.add("b", pb["terms"], unit)
    return mx_abs, pb["terms"]


def guard_wgrad(d, accumulate):
    _, t = O.wgrad(d["coef"], d["G"], d["S"], d["cs"], d["W"], d["sink"] if accumulate else None)
    GUARD.add("wgrad", t, 0.5)
    return t


def guard_colsum(x):
    GUARD.add("colsum", x.abs().sum(0))


def guard_rowdot(W, G):
    GUARD.add("rowdot", (W.double() * G.double()).abs().sum(1), limit=2.0 ** 53)


# ---------------------------------------------------------------- output layouts --------------

def prep_layout(C, K, cat):
    """The flat bf16 buffer both implementations write Wd and Mx into, PAD sentinels around
    every region: -> dict(total, wd_off, wd_len, mx_off, mx_len, ldw, ldm, arg_ldw, arg_ldm).
    cat: [Wd | Mx] rows of C + K, mx = wd + C; separate: Wd [K][C], then Mx [K][K]."""
    if cat:
        ld = C + K
        return dict(total=2 * PAD + K * ld, wd_off=PAD, wd_len=K * ld, mx_off=PAD + C, mx_len=K * ld - C, ldw=ld,
                    ldm=ld, arg_ldw=ld, arg_ldm=ld)
    return dict(total=3 * PAD + K * C + K * K, wd_off=PAD, wd_len=K * C, mx_off=2 * PAD + K * C, mx_len=K * K, ldw=C,
                ldm=K, arg_ldw=0, arg_ldm=0)


def prep_unpack(buf, C, K, lay):
    """-> (Wd [K][C], Mx [K][K], True iff every element outside the two matrices is the sentinel)"""
    buf = buf.to(F32).reshape(-1)
    k = torch.arange(K)[:, None]
    wi = lay["wd_off"] + k * lay["ldw"] + torch.arange(C)[None, :]
    mi = lay["mx_off"] + k * lay["ldm"] + torch.arange(K)[None, :]
    rest = torch.ones(buf.numel(), dtype=torch.bool)
    rest[wi.reshape(-1)] = False
    rest[mi.reshape(-1)] = False
    return buf[wi], buf[mi], bool((buf[rest] == SENT).all())


# ---------------------------------------------------------------- the fp32 twin ---------------
# numpy float64 arrays that hold fp32 values; every kernel operation is followed by r32.

def r32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def fma32(a, b, c):
    """fmaf: the product of two fp32 values is exact in fp64; the sum is rounded to 53 bits and
    then to 24, which differs from one rounding only on a near-tie (never in the exact regime)."""
    with np.errstate(all="ignore"):
        return r32(a * b + c)


def bf16_np(x):
    return rne_bf16(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def _tree(red):
    """The LDS halving tree over the last axis (PREP_NT lanes)."""
    red = red.copy()
    off = red.shape[-1] // 2
    while off > 0:
        with np.errstate(all="ignore"):
            red[..., :off] = r32(red[..., :off] + red[..., off:2 * off])
        off //= 2
    return red[..., 0]


def twin_prep(coef, W, mu, cs, rows, lay, wrong=(), probe=None):
    """bnfold_prep_kernel -> the flat buffer (sentinels kept) and b; ``probe`` (a dict) receives
    Mx before its rounding to bf16."""
    C, K = W.shape
    A, D, E = coef.reshape(3, C)
    p = prep_path(C, K)
    KW, P = p["KW"], p["P"]
    # b, first part: thread t sums its channels t, t + 1024, ..; then the tree
    eb = np.zeros((K, PREP_NT))
    for c0 in range(0, C, PREP_NT):
        c = np.arange(c0, min(C, c0 + PREP_NT))
        wl = W[c].T                                                 # [l][t]
        e = fma32(E[c][None, :], wl, eb[:, :len(c)])
        if mu is not None and "b_no_mu" not in wrong:
            with np.errstate(all="ignore"):
                m1 = -r32(r32(E[c] + r32(D[c] * mu[c])) / A[c])
                ex = r32(A[c][None, :] * wl)
                corr = fma32(m1[None, :], ex - bf16_np(ex), e)
            live = (A[c] != 0) | ("b_corr_at_A0" in wrong)
            e = np.where(live[None, :], corr, e)
        eb[:, :len(c)] = e
    bsum = _tree(eb)
    # Mx: lane group q sums the channels q, q + P, ..; the groups are added in order
    sm = W.copy() if "mx_no_D" in wrong else r32(W * D[:, None])   # [c][l]
    v = np.zeros((K, K))
    for q in range(P):
        if "mx_skip_group" in wrong and q == P - 1 and P > 1:
            continue
        acc = np.zeros((K, K))
        for c in range(q, C, P):
            acc = fma32(sm[c][:, None], W[c][None, :], acc)
        v = acc if q == 0 else r32(v + acc)
    r = bf16_np(v)
    if probe is not None:
        probe["mx_fp32"] = v
    ca = np.zeros((K, PREP_NT))
    if cs is not None and "b_no_cs" not in wrong:
        inv_rows = r32(1.0 / rows) if rows > 0 else 0.0
        for k0 in range(0, K, KW):
            ca[:, :KW] = fma32(r32(cs[k0:k0 + KW] * inv_rows)[None, :], (v - r)[:, k0:k0 + KW], ca[:, :KW])
    with np.errstate(all="ignore"):
        bias = r32(bsum + _tree(ca))
    # Wd from the transposed weights, element e of [K][C]
    wt = W.T.reshape(-1)
    if "wd_ck" in wrong:
        wt = W.reshape(-1)
    wd = bf16_np(r32(np.tile(A, K) * wt)).reshape(K, C)
    buf = np.full(lay["total"], SENT)
    ldw = C if "ldw_ignored" in wrong else lay["ldw"]
    for k in range(K):
        buf[lay["wd_off"] + k * ldw:lay["wd_off"] + k * ldw + C] = wd[k]
    for k in range(K):
        buf[lay["mx_off"] + k * lay["ldm"]:lay["mx_off"] + k * lay["ldm"] + K] = r[k]
    return buf, bias


def twin_colsum(x, wrong=()):
    """bnfold_colsum_kernel + bnfold_colsum_finish_kernel -> (cs [K], partial [512][K])"""
    rows, K = x.shape
    K8 = K // 8
    v = x.reshape(-1, 8)
    n8 = v.shape[0]
    e0 = np.arange(COLSUM_STRIDE)
    n_e = np.where(e0 < n8, -(-(n8 - e0) // COLSUM_STRIDE), 0)
    acc = np.zeros((COLSUM_STRIDE, 8))
    for j in range(-(-n8 // COLSUM_STRIDE)):
        chunk = v[j * COLSUM_STRIDE:(j + 1) * COLSUM_STRIDE]
        n = chunk.shape[0]
        if "colsum_tail_dropped" in wrong:
            chunk = np.where((j < 4 * (n_e[:n] // 4))[:, None], chunk, 0.0)
        acc[:n] = r32(acc[:n] + chunk)
    red = acc.reshape(COLSUM_BLOCKS, COLSUM_NT // K8, K8, 8)
    s = np.zeros((COLSUM_BLOCKS, K8, 8))
    for q in range(COLSUM_NT // K8):
        s = r32(s + red[:, q])
    if "colsum_group_off_by_one" in wrong:
        s = np.roll(s, -1, axis=1)
    partial = s.reshape(COLSUM_BLOCKS, K)
    lanes = np.zeros((16, K))
    for b in range(COLSUM_BLOCKS // 16):
        lanes = r32(lanes + partial[16 * b:16 * b + 16])
    cs = np.zeros(K)
    for q in range(16):
        cs = r32(cs + lanes[q])
    return cs, partial


def twin_wgrad(coef, G, S, cs, W, sink, accumulate, wrong=()):
    C, K = W.shape
    a, d, e = (t[:, None] for t in coef.reshape(3, C))
    if "wgrad_S_transposed" in wrong:
        S = S.T
    if "wgrad_first_cs_only" in wrong:
        cs = cs[:1]
    ws = np.zeros((C, K))
    for l in range(K):
        ws = fma32(W[:, l:l + 1], S[l][None, :], ws)
    sk = np.zeros(K)
    for b in range(cs.shape[0]):
        sk = r32(sk + cs[b])
    v = r32(r32(r32(a * G) + r32(d * ws)) + r32(e * sk[None, :]))
    if accumulate and "wgrad_ignores_accumulate" not in wrong:
        v = r32(sink + v)
    return v


def twin_rowdot(G, W, ns, wrong=()):
    C, K = W.shape
    acc = np.zeros((C, 64))
    for k0 in range(0, K, 64):
        n = min(64, K - k0)
        acc[:, :n] = acc[:, :n] + W[:, k0:k0 + n] * G[:, k0:k0 + n]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    hi = r32(acc[:, 0])
    lo = r32(acc[:, 0] - hi)
    if "rowdot_hi_lo_swapped" in wrong:
        hi, lo = lo, hi
    out = np.zeros((2, ns, C))
    j = 0 if "rowdot_set0" in wrong else 1
    out[0, j], out[1, j] = hi, lo
    return out


DEFECTS = ["mx_no_D", "mx_skip_group", "wd_ck", "ldw_ignored", "b_no_mu", "b_no_cs", "b_corr_at_A0",
           "colsum_tail_dropped", "colsum_group_off_by_one", "wgrad_S_transposed", "wgrad_ignores_accumulate",
           "wgrad_first_cs_only", "rowdot_hi_lo_swapped", "rowdot_set0"]


# ---------------------------------------------------------------- implementations -------------

def _np(t):
    return None if t is None else t.to(F64).numpy()


class TwinImpl:
    """The fp32 twin behind the implementation interface; ``wrong`` names deliberate defects."""

    def __init__(self, wrong=()):
        self.wrong = set(wrong)
        assert self.wrong <= set(DEFECTS), self.wrong

    def prep(self, d):
        lay = prep_layout(d["C"], d["K"], d["cat"])
        buf, bias = twin_prep(_np(d["coef"]), _np(d["W"]), _np(d["mu"]), _np(d["cs"]), d["rows"], lay, self.wrong)
        return torch.from_numpy(buf).to(F32), torch.from_numpy(bias).to(F32)

    def colsum(self, x):
        cs, partial = twin_colsum(_np(x), self.wrong)
        return torch.from_numpy(cs).to(F32), torch.from_numpy(partial).to(F32)

    def wgrad(self, d, accumulate):
        v = twin_wgrad(_np(d["coef"]), _np(d["G"]), _np(d["S"]), _np(d["cs"]), _np(d["W"]), _np(d["sink"]),
                       accumulate, self.wrong)
        return torch.from_numpy(v).to(F32), True

    def rowdot(self, G, W, ns):
        return torch.from_numpy(twin_rowdot(_np(G), _np(W), ns, self.wrong)).to(F32)


class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _f(self, t):
        return None if t is None else t.to(F32).contiguous().to(self.dev)

    def _w(self, W):        # [C][K] -> ([C][1][1][K], [K][1][1][C]) bf16
        C, K = W.shape
        w = W.to(BF16).to(self.dev)
        return w.reshape(C, 1, 1, K).contiguous(), w.T.contiguous().reshape(K, 1, 1, C)

    def prep(self, d):
        C, K = d["C"], d["K"]
        lay = prep_layout(C, K, d["cat"])
        buf = torch.full((lay["total"],), SENT, dtype=BF16, device=self.dev)
        bias = torch.full((K,), float("nan"), device=self.dev)
        w, wt = self._w(d["W"])
        self.m.bnfold_prep(self._f(d["coef"]), w, wt, mu=self._f(d["mu"]), cs=self._f(d["cs"]), rows=d["rows"],
                           ldw=lay["arg_ldw"], ldm=lay["arg_ldm"],
                           wd_out=buf[lay["wd_off"]:lay["wd_off"] + lay["wd_len"]],
                           mx_out=buf[lay["mx_off"]:lay["mx_off"] + lay["mx_len"]], bias_out=bias)
        return buf.cpu().to(F32), bias.cpu()

    def colsum(self, x):
        K = x.shape[1]
        poisoned = torch.full((COLSUM_BLOCKS, K), float("nan"), device=self.dev)
        cs, partial = self.m.bnfold_colsum(x.to(BF16).to(self.dev), partial=poisoned)
        assert partial.data_ptr() == poisoned.data_ptr()
        return cs.cpu(), partial.cpu()

    def wgrad(self, d, accumulate):
        """accumulate: the sink is a view inside a sentinel buffer; else it is NaN-filled."""
        C, K = d["C"], d["K"]
        w, _ = self._w(d["W"])
        buf = torch.full((2 * PAD + C * K,), SENT, device=self.dev)
        sink = buf[PAD:PAD + C * K].view(C, K)
        sink.copy_(self._f(d["sink"]) if accumulate else torch.full((C, K), float("nan")))
        out = self.m.bnfold_wgrad(self._f(d["coef"]), self._f(d["G"]), self._f(d["S"]), self._f(d["cs"]), w, sink,
                                  bool(accumulate))
        assert out.data_ptr() == sink.data_ptr()
        host = buf.cpu()
        intact = bool((host[:PAD] == SENT).all() and (host[PAD + C * K:] == SENT).all())
        return host[PAD:PAD + C * K].reshape(C, K).clone(), intact

    def rowdot(self, G, W, ns):
        C = W.shape[0]
        w, _ = self._w(W)
        out = torch.full((2, ns, C), float("nan"), device=self.dev)
        return self.m.bnfold_rowdot(self._f(G), w, ns, out).cpu()


# ---------------------------------------------------------------- comparison ------------------

def equal_at(name, got, ref, ctx=""):
    """torch.equal on 2-D (or 1-D) results, reporting the first differing (row, column)."""
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = ~((got == ref) & torch.isfinite(got))
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name} {ctx}: {int(bad.sum())} of {bad.numel()} values differ, first at {tuple(i)}: "
                             f"got {got[tuple(i)].item()!r}, ref {ref[tuple(i)].item()!r}")


def f32_down(x):
    f = x.to(F32)
    return torch.where(f.to(F64) > x, torch.nextafter(f, torch.full_like(f, -float("inf"))), f).to(F64)


def f32_up(x):
    f = x.to(F32)
    return torch.where(f.to(F64) < x, torch.nextafter(f, torch.full_like(f, float("inf"))), f).to(F64)


def bf16_within(stats, name, got, ref, delta, ctx=""):
    """rne_bf16(ref − δ) <= got <= rne_bf16(ref + δ); records |got − ref| / (δ + half a bf16 ulp
    of the upper end) for the report."""
    got, ref, delta = got.to(F64), ref.to(F64), delta.to(F64)
    assert torch.isfinite(got).all(), f"{name}: non-finite result {ctx}"
    lo, hi = rne_bf16(f32_down(ref - delta)), rne_bf16(f32_up(ref + delta))
    half = torch.maximum(lo.abs(), hi.abs()) * 2.0 ** -8
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (delta + half))
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), ratio.max().item())
    bad = (got < lo) | (got > hi)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name} {ctx}: {int(bad.sum())} values outside the bf16 interval, first at {i}: got "
                             f"{got[i].item()!r}, interval [{lo[i].item()!r}, {hi[i].item()!r}], ref {ref[i].item()!r}")


def check_prep(impl, name, regime, stats=None):
    d = prep_inputs(name, regime)
    C, K = d["C"], d["K"]
    ctx = f"({name}, {regime})"
    lay = prep_layout(C, K, d["cat"])
    buf, bias = impl.prep(d)
    wd, mx, intact = prep_unpack(buf, C, K, lay)
    equal_at("Wd", wd, O.prep_wd(d["coef"], d["W"]), ctx)
    mx_ref, mx_abs = O.prep_mx(d["coef"], d["W"])
    if regime == "exact":
        guard_prep(d)
        equal_at("Mx", mx, rne_bf16(mx_ref), ctx)
        equal_at("Mx symmetry", mx, mx.T, ctx)
        pb = O.prep_bias(d["coef"], d["W"], d["mu"], d["cs"], d["rows"], wd, mx)
        equal_at("b", bias, pb["b"], ctx)
    else:
        d_mx = gamma(mx_depth(C, K)) * mx_abs
        bf16_within(stats, "prep Mx", mx, mx_ref, d_mx, ctx)
        pb = O.prep_bias(d["coef"], d["W"], d["mu"], d["cs"], d["rows"], wd, mx)
        bound = gamma(bias_depth(C, K)) * pb["terms"] + U24 * pb["ex_abs"] + d_mx @ pb["mean_a2"].abs()
        within(stats, "prep b", bias, pb["b"], bound, ctx=ctx)
    assert torch.isfinite(bias).all(), f"b: non-finite {ctx}"
    assert intact, f"prep wrote outside Wd and Mx {ctx}"
    return pb


def check_colsum(impl, K, rows, regime, stats=None):
    ctx = f"(K={K}, rows={rows}, n8={rows * K // 8}, {regime})"
    x = colsum_inputs(K, rows, regime)
    cs, partial = impl.colsum(x)
    assert torch.isfinite(partial).all(), f"colsum: a row of partial was not overwritten {ctx}"
    assert torch.isfinite(cs).all(), f"colsum: cs not finite {ctx}"
    ref, ref_abs = O.colsum(x)
    pref = O.colsum_partial(x, COLSUM_BLOCKS, COLSUM_NT)
    if regime == "exact":
        guard_colsum(x)
        equal_at("colsum partial", partial, pref, ctx)
        equal_at("colsum cs", cs, ref, ctx)
    else:
        d_part, d_cs = colsum_depths(K, rows)
        pabs = O.colsum_partial(x.abs(), COLSUM_BLOCKS, COLSUM_NT)
        within(stats, "colsum partial", partial, pref, gamma(d_part) * pabs + 1e-300, ctx=ctx)
        within(stats, "colsum cs", cs, ref, gamma(d_cs) * ref_abs + 1e-300, ctx=ctx)


def check_wgrad(impl, C, K, ncs, accumulate, regime, stats=None):
    ctx = f"(C={C}, K={K}, ncs={ncs}, accumulate={accumulate}, {regime})"
    d = wgrad_inputs(C, K, ncs, regime)
    got, intact = impl.wgrad(d, accumulate)
    ref, terms = O.wgrad(d["coef"], d["G"], d["S"], d["cs"], d["W"], d["sink"] if accumulate else None)
    if regime == "exact":
        guard_wgrad(d, accumulate)
        equal_at("wgrad", got, ref, ctx)
    else:
        within(stats, "wgrad", got, ref, gamma(K + ncs + 4) * terms, ctx=ctx)
    assert intact, f"wgrad wrote outside its sink {ctx}"


def check_rowdot(impl, C, K, ns, kind, stats=None):
    ctx = f"(C={C}, K={K}, ns={ns}, {kind})"
    W, G = rowdot_inputs(C, K, kind)
    out = impl.rowdot(G, W, ns).to(F64)
    assert out.shape == (2, ns, C)
    ref, terms = O.rowdot(G, W)
    for j in [0, 2][:ns - 1]:
        assert (out[:, j] == 0).all(), f"rowdot: set {j} is not 0 {ctx}"
    hi, lo = out[0, 1], out[1, 1]
    if kind == "exact":
        guard_rowdot(W, G)
        rhi, rlo = O.hi_lo(ref)
        assert (rlo != 0).any(), "the exact rowdot case must have a non-zero lo"
        equal_at("rowdot hi", hi, rhi, ctx)
        equal_at("rowdot lo", lo, rlo, ctx)
    else:
        if kind == "cancel" and K > 1:
            assert (ref.abs() <= 2.0 ** -20 * terms).all(), "the cancellation case must cancel"
        within(stats, f"rowdot {kind}", hi + lo, ref, K * U53 * terms + U48 * ref.abs() + 1e-300, ctx=ctx)
        assert (lo.abs() <= O.ulp32(hi) / 2).all(), f"rowdot: |lo| > ulp(hi)/2 {ctx}"


def check_repeatable(impl):
    """Two calls of every operation on the same inputs: bit-identical outputs."""
    d = prep_inputs("production (512, 128)", "wide")
    a, b = impl.prep(d), impl.prep(d)
    same_bits("prep buffer", a[0], b[0])
    same_bits("prep b", a[1], b[1])
    x = colsum_inputs(64, -(-(_S + 3) // 8), "wide")
    a, b = impl.colsum(x), impl.colsum(x)
    same_bits("colsum cs", a[0], b[0])
    same_bits("colsum partial", a[1], b[1])
    d = wgrad_inputs(256, 64, 3, "wide")
    for acc in (0, 1):
        same_bits("wgrad", impl.wgrad(d, acc)[0], impl.wgrad(d, acc)[0])
    W, G = rowdot_inputs(512, 128, "wide")
    same_bits("rowdot", impl.rowdot(G, W, 3), impl.rowdot(G, W, 3))


# name -> (the comparison that must fail, the statistic that must reach 4 or None: inequality
# in the exact regime)
DEFECT_CASES = {
    "mx_no_D": (lambda i, s: check_prep(i, "(7, 64) separate", "exact", s), None),
    "mx_skip_group": (lambda i, s: check_prep(i, "production (256, 64)", "exact", s), None),
    "wd_ck": (lambda i, s: check_prep(i, "(7, 64) separate", "exact", s), None),
    "ldw_ignored": (lambda i, s: check_prep(i, "(7, 64) cat", "exact", s), None),
    "b_no_mu": (lambda i, s: check_prep(i, "corr (256, 64)", "exact", s), None),
    "b_no_cs": (lambda i, s: check_prep(i, "corr (256, 64)", "exact", s), None),
    "b_corr_at_A0": (lambda i, s: check_prep(i, "(7, 64) A = 0", "exact", s), None),
    "colsum_tail_dropped": (lambda i, s: check_colsum(i, 8, 5 * _S + 77, "exact", s), None),
    "colsum_group_off_by_one": (lambda i, s: check_colsum(i, 64, -(-255 // 8), "exact", s), None),
    "wgrad_S_transposed": (lambda i, s: check_wgrad(i, 5, 72, 3, 0, "exact", s), None),
    "wgrad_ignores_accumulate": (lambda i, s: check_wgrad(i, 1, 8, 3, 1, "exact", s), None),
    "wgrad_first_cs_only": (lambda i, s: check_wgrad(i, 5, 72, 3, 0, "exact", s), None),
    "rowdot_hi_lo_swapped": (lambda i, s: check_rowdot(i, 7, 100, 2, "exact", s), None),
    "rowdot_set0": (lambda i, s: check_rowdot(i, 7, 100, 3, "exact", s), None),
}
# the same defects in the wide regime, where a bound has to catch them: (comparison, statistic)
DEFECT_CASES_WIDE = {
    "b_no_mu": (lambda i, s: check_prep(i, "production (256, 64)", "wide", s), "prep b"),
    "b_no_cs": (lambda i, s: check_prep(i, "production (256, 64)", "wide", s), "prep b"),
    "colsum_tail_dropped": (lambda i, s: check_colsum(i, 8, 5 * _S + 77, "wide", s), "colsum partial"),
    "wgrad_S_transposed": (lambda i, s: check_wgrad(i, 5, 72, 3, 0, "wide", s), "wgrad"),
    "wgrad_ignores_accumulate": (lambda i, s: check_wgrad(i, 1, 8, 3, 1, "wide", s), "wgrad"),
    "wgrad_first_cs_only": (lambda i, s: check_wgrad(i, 5, 72, 3, 0, "wide", s), "wgrad"),
}
