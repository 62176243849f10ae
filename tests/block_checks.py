"""Cases, inputs, bounds, implementations and comparison functions of the residual-block tests.

The comparison functions take an *implementation* with two methods, ``fwd`` and ``bwd``, that map
CPU tensors to CPU tensors. ``ExtImpl`` calls the executor (``block_fwd`` / ``block_bwd`` of
csrc/bindings/block_ops.cpp); ``TwinImpl`` is a CPU twin of the executor's sequencing (the
stage functions of tests/block_oracle.py with a float32 cast or ``rne_bf16`` at every storage
point), optionally with a named deliberate defect (``DEFECTS``). tests/test_block_oracle.py
holds the twin to every comparison with the allowances for fp32 arithmetic (u22·T, γ(n)·Σ|term|)
halved - the reach of a single bf16 or fp32 rounding cannot be halved - and shows each defect
caught at its named case; tests/test_gpu_block_oracle.py holds the executor to the same comparisons.

Every comparison is teacher forced: an oracle stage is fed the tensors the implementation
itself stored, so each check spans one stored tensor (or two, where the tensor in between is
not observable) and no error accumulates along the block.

Forward. ``block_fwd`` returns every intermediate, so each slot is compared with ONE oracle
stage applied to the returned slots it was computed from.

Backward. ``block_bwd`` is a pure function of its arguments, so the test builds ``saved``,
``bnst``, the weights and the sinks itself; they are not a consistent forward. The activations
x, a1, a2 are read by the weight gradients only, and here they are ONE-HOT: pixel p carries
e_p (all shapes have rows <= channels, asserted). The weight-gradient sink of a conv is then a
copy of that conv's output gradient (the *transcript*):

    dW[k, centre, centre, flat(n, p·s, q·s)] = dy[n, p, q, k]

one product plus zeros, exact in any wgrad family and any split. The transcript entries of a
sink start from +0, because fp32(sink + bf16) is not exact for |dy| < 2^-14·|sink|; every other
entry starts from a non-zero dyadic value and must come back as sink + (one product), to
2·u24·(|sink| + |product|): that is where ``+=`` is checked.

Bounds. u8 = 2^-8, u22 = 2^-22, u24 = 2^-24, γ(n) = n·u24 / (1 − n·u24).

  conv / dgrad store   s = the fp64 value, mag = Σ|a·b| of its terms, δ = γ(Kdim)·mag (Kdim =
                       R·S·C fp32 accumulations in any order); the stored bf16 lies in
                       [bf16(s − δ), bf16(s + δ)] (rounding is monotone).
  second rounding      dx = bf16(bf16(acc) + addend): the interval end points are added and
                       rounded again, addend exact (dout·mask) or itself an interval (the
                       shortcut's data gradient).
  conv statistics      the slab sums the fp32 accumulators: |ΔΣy| <= Σδ + γ(rows + 2)·Σ|s|,
                       |ΔΣy²| <= Σ(2·|s|·δ + δ²) + γ(rows + 3)·Σs² (any order of rows terms,
                       the square, the accumulator's own rounding).
  finalize             bn_checks.finalize_bounds around the oracle's value for the oracle's
                       sums, plus the sums' error carried through: Δmean = ΔΣy/n,
                       Δvar = ΔΣy²/n + 2·|mean|·Δmean + Δmean², Δinvstd <= Δvar / (2·(var − Δvar
                       + eps)^1.5) (invstd is convex and decreasing in var), Δscale =
                       |γ|·Δinvstd, Δshift = |γ|·(|mean|·Δinvstd + invstd·Δmean + Δmean·Δinvstd),
                       Δrunning_mean = m·Δmean, Δrunning_var = m·Δvar·n/(n − 1). The count n
                       is stated per BN by ``Spec.bn_rows``.
  bn_apply, out        u8·|z| + u22·T, z and T from the kernel's own scale and shift
                       (bn_checks). With fold_fwd y3 is not stored, but the epilogue applies
                       the BN to bf16(acc3) (igemm_kernel.h, FWD VAR 2), i.e. to the value a
                       stored y3 would hold: some y3 in [bf16(s3 − δ3), bf16(s3 + δ3)]. z and T
                       from y3r = bf16(s3), and with w = the interval's reach from y3r (0 unless
                       s3 lies within δ3 of a rounding boundary) the bound grows by
                       (1 + u8 + u22)·|scale|·w.
  output-BN backward   sums: bn_checks.reduce_bound; from a slab: rows·2^-52·Σ|slab|. A, D, E,
                       dγ, dβ: bn_checks.coef_bounds with those. dy (transcript): with
                       pert = |ΔA|·|dz| + |ΔD|·|y| + |ΔE|,  u8·(|z| + pert) + u22·(T + pert) + pert.
  dgrad -> BN backward (two stages: da is not observable) da = bf16(fp32 acc):
                       Δda = δ + u8·(|acc| + δ). The sums are taken from the stored da in
                       fp32: ΔΣ0 = ΣΔda·m + γ(rows + 3)·Σ(|da| + Δda)·m and ΔΣ1 the same with
                       the factor |y − μ| (any order of rows terms, y − μ, the product); they
                       enter coef_bounds. dy: pert = (|A| + |ΔA|)·Δda·m + |ΔA|·|da|·m + |ΔD|·|y|
                       + |ΔE|, then as above.
  folded dgrad         (BN3 fold, tests/bnfold_checks.py for the single kernels) da2 = bf16(dz·Wd +
                       a2·Mx + b), one rounding, against the unfolded fp64 dy3·W3 with dy3 = A·dz +
                       D·(a2·W3ᵀ) + E. δ = u·Σ_c(|dz| + |mean dz|)·|A·W3|       Wd = bf16(A·W3), and the
                                                                            row-mean part b takes back
                         + Σ_k(|a2| + |mean a2|)·η,  η = u8·|Mx| + (1 + u8)·γ(mx_depth)·Σ|W·D·W|
                         + γ(bias_depth)·Σ|terms of b| + u24·Σ|mean dz·A·W3|
                         + Σ_c(|ΔA|·|dz| + |ΔD|·|y3| + |ΔE|)·|W3|           the coefficients' own bounds
                         + γ(C + K + 2)·Σ|terms of the GEMM|
                         + u8·|T| + u24·|T|  (non-concatenated form only: T = bf16(a2·Mx + b) is
                           stored, then added to the accumulators in fp32, before the one rounding)
                       with u = u8 + 8·u24 (the bf16 rounding of a fp32 product, and mean dz taken
                       from fp32 coefficients). δ then enters the two-stage bound above in place
                       of the plain dgrad's. The same for a folded stride-1 shortcut, whose
                       result is the final dgrad's addend interval.
  folded dW            bnfold_checks' wgrad bound γ(K + 5)·Σ|term| plus the coefficients' bounds
                       on each term; the one-hot input makes G, S and Σa2 exact.
  rowdot rows          bnfold_checks' rowdot bound on hi + lo; sets 0 and 2 of the two rows zero;
                       all other rows of in_slab bitwise unchanged.
  prev_slab            from the stored dx (exact input): γ(rows + 3)·Σ|term| per set.
  masked store         the unmasked dx of a second call times the mask: kept elements bit-equal,
                       dropped elements zero.

On tightness: the bounds whose leading term is u8·|z| (conv store, bn_apply, dy, dx) are
one-rounding intervals. A correctly rounded bf16 store errs by up to 2^-8·|z| just above a power
of two, so a correct kernel reaches error / bound close to 1 at some element by construction, in
any order of operations; the fp32 allowance lies on top of that and is what a reordering moves.

The recomputed masks (y·sc + sh > 0) are decided in fp32 by the kernels and in fp64 here; the
inputs satisfy ``bn_checks.mask_margin_ok`` (asserted for every case), so no element is left
out of any comparison. No tolerance comes from a measurement, except bn_eval_affine's, which is
bn_checks.EVAL_AFFINE_TOL.
"""
from __future__ import annotations

import numpy as np
import torch

import block_oracle as O
import bnfold_checks as FC
import bnfold_oracle as BO
import bn_checks as BC
import bn_oracle as B
import conv_oracle as C
from bn_checks import within
from bnfold_checks import f32_down, f32_up, gamma
from conv_oracle import rne_bf16

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U8, U22, U24, U52 = BC.U8, BC.U22, BC.U24, BC.U52
EPS, MOMENTUM = BC.EPS, BC.MOMENTUM

# ---------------------------------------------------------------- case tables -----------------
KINDS = {
    "basic_id": O.Spec(False, False, 1, 64, 64, 64),
    "basic_proj_s2": O.Spec(False, True, 2, 64, 128, 128),
    "bott_id": O.Spec(True, False, 1, 256, 64, 256),
    "bott_proj_s1": O.Spec(True, True, 1, 64, 64, 256),
    "bott_proj_s2": O.Spec(True, True, 2, 64, 64, 256),
}
# The fold's data-gradient operand has two forms (fold_dgrad_operands, block_ops.cpp):
# K-concatenated when C3 / K3 is a power of two (every width above), else Wd with T = bf16(a2·Mx
# + b) added to the accumulators. The second is reached at rows <= channels too, with C3 = 3·K3,
# so it keeps its transcripts and needs no larger case: an identity bottleneck 192 -> 64 -> 192,
# run in the fold modes only.
NONCAT_KIND = "bott_id_w192"
KINDS_FOLD_ONLY = {NONCAT_KIND: O.Spec(True, False, 1, 192, 64, 192)}
SHAPES = {"2x4x4": (2, 4, 4), "3x3x3": (3, 3, 3)}       # 32 rows; 27 rows, P = 2 under stride 2
FWD_MODES = ["train", "train_fold_fwd", "eval"]
# backward: no slab (elementwise source, bitmask out) | in_slab given (2 sets identity, 3 sets
# projection) | prev with one / two statistics sets | prev with the fold marker (masked store) |
# prev without y3 (two extra slab rows)
BWD_MODES = ["noslab", "slab", "prev1", "prev2", "prev_masked", "prev_noy"]
CASES = [(k, s) for k in KINDS for s in SHAPES]
KINDS.update(KINDS_FOLD_ONLY)


def masked_store_applies(kind):
    """The masked store is a mode of a stride-1 final dgrad (conv_dgrad_bnstat refuses it
    otherwise): the block's first conv must have stride 1. A strided BasicBlock follows a
    BasicBlock, which never folds, so the executor is never asked for it there."""
    spec = KINDS[kind]
    return spec.bottleneck or spec.stride == 1


# BN3 fold of a bottleneck's backward (in_slab given, dout already masked): fold_w = [W3] |
# [W3, Ws] (stride-1 projection) | the same with the forward-time Grams appended (length 3, or 6
# on the stride-1 projection) | [W3] with saved[kY3] empty (bnfold_rowdot fills two slab rows)
FOLD_MODES = ["fold", "fold_sc", "fold_gram", "no_y3"]


def fold_applies(kind, mode):
    spec = KINDS[kind]
    return spec.bottleneck and (mode != "fold_sc" or (spec.proj and spec.stride == 1))


def fold_spec(kind, mode):
    """-> dict(n: folded convs, grams, no_y3) of a fold mode, None otherwise."""
    if mode not in FOLD_MODES:
        return None
    spec = KINDS[kind]
    two = spec.proj and spec.stride == 1 and mode in ("fold_sc", "fold_gram")
    return dict(n=2 if two else 1, grams=mode == "fold_gram", no_y3=mode == "no_y3")


def dgrad_cat_supported(K, cat_ch):
    """Mirror of sdx_plan::dgrad_cat_supported (csrc/include/conv_plan.h) for a stride-1 1x1
    dgrad with K gradient channels and cat_ch concatenated ones, default knobs."""
    if cat_ch <= 0 or K % 64 or cat_ch % 64 or K % cat_ch:
        return False
    r = K // cat_ch
    return r & (r - 1) == 0


def chain_dgrads(kind, shape):
    """The data gradients block_bwd issues for a case, as conv_plan requests: (name, (N, H, W, C,
    K, R, S, stride, pad) with H x W the dgrad's OUTPUT grid, bnstat, cat_ch)."""
    spec, N, H, W, P, Q = geometry(kind, shape)
    hw = conv_inputs_hw(spec, N, H, W)
    out = []
    for i in range(spec.nconv - 1, -1, -1):
        K, R, Cc, s, p = spec.convs[i]
        # every dgrad of the chain carries the BN-statistics epilogue: conv i > 0 for the BN
        # before it, conv 0 for the previous block (when prev is given)
        out.append((f"conv{i + 1}", (N, hw[i][0], hw[i][1], Cc, K, R, R, s, p), True, 0))
    if spec.bottleneck:
        out.append(("conv3 folded", (N, P, Q, spec.mid, spec.cout, 1, 1, 1, 0), True, spec.mid))
    if spec.proj:
        if spec.stride > 1:      # SDX_SUB_ADDEND: a compact stride-1 dgrad on the P x Q grid
            out.append(("shortcut compact", (N, P, Q, spec.cin, spec.cout, 1, 1, 1, 0), False, 0))
        else:
            out.append(("shortcut", (N, H, W, spec.cin, spec.cout, 1, 1, 1, 0), False, 0))
            if spec.bottleneck:
                out.append(("shortcut folded", (N, H, W, spec.cin, spec.cout, 1, 1, 1, 0), False, spec.cin))
    return out


def check_paths(m, kind, shape):
    """Which path each launch of the case takes, from conv_plan (host only). Every dgrad is a
    launch the launcher accepts: an implicit GEMM, or the tap-reuse tile for a stride-1 3x3 on
    4x4 images. A strided one
    merges its stride² sub-pixel classes into one launch, a stride-1 one has a single class, the
    folded ones take the K-concatenated form, and every weight gradient is planned."""
    spec, N, H, W, P, Q = geometry(kind, shape)
    for name, g, bnstat, cat in chain_dgrads(kind, shape):
        d = m.conv_plan(*g, True, full=True, kind="dgrad", bnstat=bnstat, cat_ch=cat)
        ctx = f"({kind}, {shape}, {name}): {d}"
        st = g[7]
        # the two shapes split the stride-1 3x3 dgrads between the two conv families: 4x4 images
        # fill a tap-reuse tile (cfg 13, whole images per 128-row tile), 3x3 images do not
        tap = g[5] == 3 and st == 1 and (g[1], g[2]) == (4, 4)
        assert d["ok"] and bool(any(d["tap"])) == tap and (d["cfg"] == 13 if tap else d["cfg"] in range(7)), ctx
        assert d["merged"] == (st > 1) and len(d["class_mt"]) == st * st, ctx
        assert d["mt"] == sum(d["class_mt"]), ctx
        if cat:
            assert dgrad_cat_supported(g[4], cat), ctx
    hw = conv_inputs_hw(spec, N, H, W)
    for i, (K, R, Cc, s, p) in enumerate(spec.convs):
        d = m.conv_plan(N, hw[i][0], hw[i][1], Cc, K, R, R, s, p, False, full=True, kind="wgrad", accumulate=True)
        assert d["ok"], f"({kind}, {shape}, wgrad {i}): {d}"


BWD_CASES = [(k, s, m) for k, s in CASES for m in BWD_MODES
             if masked_store_applies(k) or m not in ("prev_masked", "prev_noy")] + \
            [(k, s, m) for k, s in CASES for m in FOLD_MODES if fold_applies(k, m)] + \
            [(NONCAT_KIND, s, m) for s in SHAPES for m in ("fold", "fold_gram", "no_y3")]
BWD_REFUSED = [(k, s, m) for k, s in CASES for m in ("prev_masked", "prev_noy") if not masked_store_applies(k)]


def geometry(kind, shape):
    spec = KINDS[kind]
    N, H, W = SHAPES[shape]
    P, Q = spec.out_hw(H, W)
    return spec, N, H, W, P, Q


def onehot_ok(kind, shape):
    """rows <= channels for x, a1 and a2."""
    spec, N, H, W, P, Q = geometry(kind, shape)
    ok = N * H * W <= spec.cin
    ok = ok and (N * H * W if spec.bottleneck else N * P * Q) <= spec.mid
    return ok and (not spec.bottleneck or N * P * Q <= spec.mid)


# ---------------------------------------------------------------- inputs ----------------------

def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * sum(ord(c) for c in str(k)) for i, k in enumerate(key)) % (2 ** 31))
    return g


def _bf(t):
    return t.to(BF16).to(F64)


def _dyadic(shape, g):
    """Non-zero dyadic values ±{0.5, 1, 2}."""
    v = torch.tensor([0.5, 1.0, 2.0, -0.5, -1.0, -2.0])
    return v[torch.randint(0, 6, shape, generator=g)].to(F32)


def _weights(spec, g):
    return [_bf(torch.randn(K, R, R, Cc, generator=g) / (R * R * Cc) ** 0.5) for K, R, Cc, s, p in spec.convs]


_cache = {}


def fwd_inputs(kind, shape):
    key = ("fwd", kind, shape)
    if key not in _cache:
        spec, N, H, W, P, Q = geometry(kind, shape)
        g = _gen(kind, shape, 1)
        bns = []
        for K, R, Cc, s, p in spec.convs:
            ga, be, _ = BC.channel_vectors(K, g)
            rm = (torch.randint(-8, 9, (K,), generator=g) / 8.0).to(F32)         # dyadic, non-trivial
            rv = (0.5 + torch.randint(0, 17, (K,), generator=g) / 16.0).to(F32)
            bns += [ga, be.to(F32), rm, rv]
        _cache[key] = dict(spec=spec, x=_bf(BC._with_zeros(torch.randn(N, H, W, spec.cin, generator=g), g)),
                           ws=_weights(spec, g), bns=bns)
    return _cache[key]


def _onehot(N, H, W, Cn):
    t = torch.zeros(N * H * W, Cn, dtype=F64)
    t[torch.arange(N * H * W), torch.arange(N * H * W)] = 1.0
    return t.reshape(N, H, W, Cn)


def conv_inputs_hw(spec, N, H, W):
    """(H, W) of the input of each conv."""
    P, Q = spec.out_hw(H, W)
    hw = [(H, W), (H, W) if spec.bottleneck else (P, Q)]
    if spec.bottleneck:
        hw.append((P, Q))
    if spec.proj:
        hw.append((H, W))
    return hw


def bwd_inputs(kind, shape):
    """The arguments of one block_bwd call, mode-independent part plus every mode's extras."""
    key = ("bwd", kind, shape)
    if key in _cache:
        return _cache[key]
    spec, N, H, W, P, Q = geometry(kind, shape)
    g = _gen(kind, shape, 2)
    hw_in = conv_inputs_hw(spec, N, H, W)
    d = dict(spec=spec, kind=kind, shape=shape)
    d["ins"] = [_onehot(N, h, w, spec.convs[i][2]) for i, (h, w) in enumerate(hw_in)]   # x, a1, (a2), (x)
    d["x"] = d["ins"][0]
    d["y"], d["st"], d["gamma"], d["dg"], d["db"] = [], [], [], [], []
    for i, (K, R, Cc, s, p) in enumerate(spec.convs):
        h, w = hw_in[i]
        ph, pw = C.out_size(h, R, s, p), C.out_size(w, R, s, p)
        y = BC._with_zeros(torch.randn(N, ph, pw, K, generator=g) * 2 + 0.5, g)
        sc, sh, mu = BC.channel_vectors(K, g)
        sh = torch.where(torch.arange(K) % 5 == 0, torch.zeros(()), sh).to(F32)
        d["y"].append(_bf(y))
        d["st"].append(dict(sc=sc, sh=sh, mu=mu.to(F32), iv=(torch.rand(K, generator=g) + 0.5).to(F32)))
        d["gamma"].append(BC.channel_vectors(K, g)[0])
        d["dg"].append(_dyadic((K,), g))
        d["db"].append(_dyadic((K,), g))
    d["ws"] = _weights(spec, g)
    d["wt"] = [O.dgrad_layout(w) for w in d["ws"]]
    d["dout"] = _bf(BC._with_zeros(torch.randn(N, P, Q, spec.cout, generator=g), g))
    d["bits"] = B.relu_bits(BC._with_zeros(torch.randn(N, P, Q, spec.cout, generator=g), g))
    # weight-gradient sinks: non-zero dyadic, +0 at the transcript entries
    d["dw"] = []
    for i, (K, R, Cc, s, p) in enumerate(spec.convs):
        sink = _dyadic((K, R, R, Cc), g)
        sink[:, R // 2, R // 2, transcript_cols(spec, i, N, H, W)] = 0.0
        d["dw"].append(sink)
    ns = 3 if spec.proj else 2
    d["in_slab"] = (torch.randn(5, ns, spec.cout, generator=g) * 3).to(F32)
    # the previous block (its output is x): y_last, mean_last, y_short, mean_short, out bits
    d["prev"] = dict(ya=_bf(torch.randn(N, H, W, spec.cin, generator=g)), ma=torch.randn(spec.cin, generator=g),
                     yb=_bf(torch.randn(N, H, W, spec.cin, generator=g) - 1), mb=torch.randn(spec.cin, generator=g),
                     bits=B.relu_bits(torch.randn(N, H, W, spec.cin, generator=g)))
    _cache[key] = d
    return d


def transcript_cols(spec, i, N, H, W):
    """Columns (input channels = flat input pixels) of conv i's sink that hold its transcript,
    in the order of the output pixels (n, p, q)."""
    K, R, Cc, s, p = spec.convs[i]
    h, w = conv_inputs_hw(spec, N, H, W)[i]
    ph, pw = C.out_size(h, R, s, p), C.out_size(w, R, s, p)
    n, pp, qq = torch.meshgrid(torch.arange(N), torch.arange(ph), torch.arange(pw), indexing="ij")
    return ((n * h + pp * s) * w + qq * s).reshape(-1)


def transcript(spec, i, dw_before, dw_after, N, H, W):
    """dy of conv i as [N, P, Q, K] float64 (exact bf16 values) from its sink."""
    K, R, Cc, s, p = spec.convs[i]
    h, w = conv_inputs_hw(spec, N, H, W)[i]
    ph, pw = C.out_size(h, R, s, p), C.out_size(w, R, s, p)
    cols = transcript_cols(spec, i, N, H, W)
    assert (dw_before[:, R // 2, R // 2, cols] == 0).all()
    t = dw_after[:, R // 2, R // 2, cols].to(F64).t().reshape(N, ph, pw, K).contiguous()
    assert torch.isfinite(t).all(), f"transcript of conv {i}: non-finite"
    B.bf16_bits(t)          # asserts that every value is a bf16 value: a copy, not a sum
    return t


def margins_ok(kind, shape):
    d = bwd_inputs(kind, shape)
    return all(BC.mask_margin_ok(dict(ya=y.reshape(-1, y.shape[-1]), msc=s["sc"], msh=s["sh"]))
               for y, s in zip(d["y"], d["st"]))


def bwd_args(kind, shape, mode):
    d = bwd_inputs(kind, shape)
    a = dict(d, in_slab=None, prev=None, fold=fold_spec(kind, mode))
    if mode == "slab" or a["fold"] is not None:
        a["in_slab"] = d["in_slab"]
    if mode.startswith("prev"):
        p = dict(d["prev"], two=mode == "prev2", masked=mode in ("prev_masked", "prev_noy"), noy=mode == "prev_noy")
        a["prev"] = p
    return a


# ---------------------------------------------------------------- implementations -------------
DEFECTS = ["proj_bn_input_rows", "residual_after_relu", "mask_before_residual", "dbeta3_to_shortcut_sink",
           "biased_running_var", "momentum_on_old", "dgamma_overwritten", "subgrid_offset_1_1", "shortcut_dx_dropped",
           "store_masked_ignored", "bn2_mean_for_bn1", "eval_batch_stats", "third_slab_set_missing",
           "extra_rows_first", "fold_E_missing", "fold_gram_of_x"]


def r32(t):
    return t.to(F64).to(F32).to(F64)


def rb(t):
    return rne_bf16(r32(t))


def _rows(t):
    return t.reshape(-1, t.shape[-1])


class TwinImpl:
    """CPU twin of the executor's sequencing; ``wrong`` names deliberate defects (DEFECTS)."""

    def __init__(self, wrong=()):
        self.wrong = set(wrong)
        assert self.wrong <= set(DEFECTS)

    def fwd(self, a, training, fold_fwd):
        spec, x, ws = a["spec"], a["x"], a["ws"]
        N, H, W, _ = x.shape
        bns = [t.clone() for t in a["bns"]]
        fold_fwd = fold_fwd and training and spec.bottleneck
        acc, y, act, st = [None] * spec.nbn, [None] * spec.nbn, [], [None] * spec.nbn

        def bn(i):
            g, b, rm, rv = bns[4 * i:4 * i + 4]
            count = spec.bn_rows(i, N, H, W)
            if i == spec.nconv and spec.stride > 1 and "proj_bn_input_rows" in self.wrong:
                count = N * H * W
            if not training and "eval_batch_stats" not in self.wrong:
                sc, sh = B.twin_eval_affine(g, b, rm, rv, EPS)
                return dict(scale=sc, shift=sh, mean=None, invstd=None)
            f = B.twin_finalize(B.stats(acc[i]), count, g, b, EPS, MOMENTUM, rm, rv,
                                {"biased_var"} if "biased_running_var" in self.wrong else ())
            if training:
                if "momentum_on_old" in self.wrong:
                    f["running_mean"] = (MOMENTUM * rm + (1 - MOMENTUM) * f["mean"]).to(F32)
                bns[4 * i + 2], bns[4 * i + 3] = f["running_mean"], f["running_var"]
            return f

        def conv(i, inp):
            K, R, Cc, s, p = spec.convs[i]
            acc[i] = r32(C.fwd_acc(inp, ws[i], s, p))
            y[i] = rne_bf16(acc[i])

        cur = x
        for i in range(spec.nconv):
            conv(i, cur)
            st[i] = bn(i)
            if i < spec.nconv - 1:
                cur = B.twin_apply(_rows(y[i]), st[i]["scale"], st[i]["shift"]).to(F64).reshape(y[i].shape)
                act.append(cur)
        L, n = spec.nconv - 1, spec.nconv
        ylast = y[L]            # fold_fwd: the epilogue applies the BN to bf16(acc3), y3 is only not stored
        if spec.proj:
            conv(n, x)
            st[n] = bn(n)
            r, sc2, sh2, mode = y[n], st[n]["scale"], st[n]["shift"], 1
        else:
            r, sc2, sh2, mode = x, None, None, 2
        sc, sh = st[L]["scale"], st[L]["shift"]
        if "residual_after_relu" in self.wrong:
            res = _rows(r).to(F32) * sc2 + sh2 if mode == 1 else _rows(r).to(F32)
            out = B.bf16_round(B.twin_apply(_rows(ylast), sc, sh, relu=True) + res)
        else:
            out = B.twin_apply(_rows(ylast), sc, sh, _rows(r), sc2, sh2, mode, True)
        bits = None
        if training:
            bits = B.relu_bits(B.twin_apply(_rows(ylast), sc, sh, relu=False)
                               if "mask_before_residual" in self.wrong else out)
        if fold_fwd:
            y[L] = None
        return dict(out=out.to(F64).reshape(acc[L].shape), y=y, a=act, bits=bits,
                    st=[dict(scale=s["scale"], shift=s["shift"], mean=s["mean"], invstd=s["invstd"]) for s in st],
                    rm=[bns[4 * i + 2] for i in range(spec.nbn)], rv=[bns[4 * i + 3] for i in range(spec.nbn)])

    def bwd(self, a):
        spec, x, dout = a["spec"], a["x"], a["dout"]
        N, H, W, _ = x.shape
        P, Q = spec.out_hw(H, W)
        L, n = spec.nconv - 1, spec.nconv
        wrong = self.wrong
        dw = [t.clone() for t in a["dw"]]
        dg = [t.clone() for t in a["dg"]]
        db = [t.clone() for t in a["db"]]
        st, y, ins, wt = a["st"], a["y"], a["ins"], a["wt"]
        cw = {"overwrite_sinks"} if "dgamma_overwritten" in wrong else ()

        def coef(i, sums, count, set_index=0):
            c = B.twin_coef(sums, count, a["gamma"][i], st[i]["mu"], st[i]["iv"], 1.0, set_index, dg[i], db[i], cw)
            if "dgamma_overwritten" in wrong:
                c["dbeta"] = c["dbeta"] + db[i]          # only dγ is overwritten
            dg[i], db[i] = c["dgamma"], c["dbeta"]
            return c["coef"]

        def wgrad(i, dy):
            K, R, Cc, s, p = spec.convs[i]
            dw[i] = (dw[i].to(F64) + C.wgrad(dy, ins[i], R, R, s, p)).to(F32)

        fold = a["fold"]
        ms = None if fold else ("bits", a["bits"])        # fold: dout is dz, already masked
        yL, ys = _rows(y[L]), (_rows(y[n]) if spec.proj else None)
        cntL = N * P * Q
        slab_after = None
        if a["in_slab"] is not None:
            slab_after = a["in_slab"].clone()
            if fold and fold["no_y3"]:
                W3 = a["ws"][2].reshape(spec.cout, spec.mid)
                v, _ = BO.rowdot(_rows(dout).t() @ _rows(ins[2]), W3)
                hi, lo = BO.hi_lo(v)
                at = slice(0, 2) if "extra_rows_first" in wrong else slice(slab_after.shape[0] - 2, None)
                slab_after[at] = 0.0
                slab_after[at, 1] = torch.stack([hi, lo]).to(F32)
            sums = slab_after.to(F64).sum(0)
        else:
            sums = B.twin_bwd_sums(_rows(dout), ms, yL, st[L]["mu"], ys, st[n]["mu"] if spec.proj else None,
                                   BC.bn_bwd_reduce_blocks(dout.numel()))
        db_sc_before = db[n].clone() if spec.proj else None
        db_l_before = db[L].clone()
        ca = coef(L, sums, cntL)
        cb = coef(n, sums, cntL, 1) if spec.proj else None
        if spec.proj and "dbeta3_to_shortcut_sink" in wrong:
            db[n] = db_sc_before + (db[L] - db_l_before)
            db[L] = db_l_before
        def fold_conv(i, coef_t, src, gram_src=None):
            """conv i's folded dgrad (stored bf16) and its folded weight gradient into the sink."""
            Kc, R, Cc, s, p = spec.convs[i]
            W = a["ws"][i].reshape(Kc, Cc)
            cf = coef_t.to(F64).clone()
            dz2, in2 = _rows(dout), _rows(src)
            g2 = _rows(gram_src if gram_src is not None else src)
            G, S, cs = dz2.t() @ in2, g2.t() @ g2, g2.sum(0)
            cw3 = cf.clone()
            if "fold_E_missing" in wrong:
                cw3[2] = 0.0
            dw[i] = (dw[i].to(F64) + BO.wgrad(cw3, G, S, cs[None], W)[0].reshape(dw[i].shape)).to(F32)
            wd = BO.prep_wd(cf, W)
            mx = rb(BO.prep_mx(cf, W)[0])
            bias = r32(BO.prep_bias(cw3, W, st[i]["mu"], cs if fold["grams"] else None, in2.shape[0], wd, mx)["b"])
            if not dgrad_cat_supported(Kc, Cc):
                return rb(dz2 @ wd.t() + rb(in2 @ mx.t() + bias)).reshape(src.shape)
            return rb(dz2 @ wd.t() + in2 @ mx.t() + bias).reshape(src.shape)

        if fold:
            dys = None
            if spec.proj and fold["n"] == 1:
                dys = B.twin_bwd_apply(_rows(dout), None, ys, cb)["dya"].to(F64).reshape(dout.shape)
        else:
            r = B.twin_bwd_apply(_rows(dout), ms, yL, ca, ys, cb)
            dyl = r["dya"].to(F64).reshape(dout.shape)
            dys = r["dyb"].to(F64).reshape(dout.shape) if spec.proj else None
            cur = dyl
        for i in range(L, 0, -1):
            K, R, Cc, s, p = spec.convs[i]
            if fold and i == L:
                da = fold_conv(L, ca, ins[L], x if "fold_gram_of_x" in wrong else None)
            else:
                wgrad(i, cur)
                da = rb(C.dgrad_acc(cur, wt[i], ins[i].shape[1], ins[i].shape[2], s, p))
            j = i - 1
            mj = ("affine", st[j]["sc"], st[j]["sh"])
            mu = st[1]["mu"] if (j == 0 and "bn2_mean_for_bn1" in wrong) else st[j]["mu"]
            sums_j, _, _ = B.bwd_sums(_rows(da), mj, _rows(y[j]), mu)
            cj = coef(j, sums_j, spec.bn_rows(j, N, H, W))
            cur = B.twin_bwd_apply(_rows(da), mj, _rows(y[j]), cj)["dya"].to(F64).reshape(da.shape)
        K, R, Cc, s, p = spec.convs[0]
        wgrad(0, cur)
        acc1 = rb(C.dgrad_acc(cur, wt[0], H, W, s, p))
        if fold and fold["n"] == 2:
            add = fold_conv(n, cb, x)
        elif spec.proj:
            wgrad(n, dys)
            if spec.stride > 1:
                dxs = rb(C.dgrad_acc(dys, wt[n], P, Q, 1, 0))
                add = torch.zeros_like(acc1)
                if "subgrid_offset_1_1" in wrong:
                    k1, k2 = len(range(1, H, spec.stride)), len(range(1, W, spec.stride))
                    add[:, 1::spec.stride, 1::spec.stride] = dxs[:, :k1, :k2]
                else:
                    add[:, ::spec.stride, ::spec.stride] = dxs
            else:
                add = rb(C.dgrad_acc(dys, wt[n], H, W, 1, 0))
            if "shortcut_dx_dropped" in wrong:
                add = torch.zeros_like(acc1)
        else:
            add = dout if fold else dout * C.unpack_bits(a["bits"], dout.shape)
        dx = rb(acc1 + add)
        slab = None
        if a["prev"] is not None:
            pv = a["prev"]
            mask = ("bits", pv["bits"])
            d, terms = C.bn_terms(dx, mask, None if pv["noy"] else pv["ya"], pv["ma"],
                                  pv["yb"] if pv["two"] else None, pv["mb"] if pv["two"] else None)
            slab = terms.sum(1, keepdim=True).permute(1, 0, 2)                # [1, ns, C]
            if pv["two"] and "third_slab_set_missing" in wrong:
                slab[:, 2] = 0.0
            if pv["noy"]:
                slab = torch.cat([slab, torch.zeros(2, *slab.shape[1:], dtype=F64)])
            slab = slab.to(F32)
            if pv["masked"] and "store_masked_ignored" not in wrong:
                dx = d
        return dict(dx=dx, prev_slab=slab, dw=dw, dg=dg, db=db, in_slab=slab_after)


class ExtImpl:
    """The executor of the extension module ``m`` on device ``dev``; ``side``: a HIP stream
    handle for the side-stream work (0: everything on the current stream)."""

    def __init__(self, m, dev, side=0):
        self.m, self.dev, self.side = m, dev, side

    def _b(self, t):
        return t.to(BF16).contiguous().to(self.dev)

    def _v(self, t):
        return t.to(F32).contiguous().to(self.dev)

    @staticmethod
    def _c(t):
        return None if t is None or t.numel() == 0 else t.cpu().to(F64)

    def fwd(self, a, training, fold_fwd):
        spec = a["spec"]
        bn = [self._v(t).clone() for t in a["bns"]]
        x, ws = self._b(a["x"]), [self._b(w) for w in a["ws"]]
        keep = [t.clone() for t in [x] + ws]
        r = self.m.block_fwd(x, ws, bn, spec.stride, spec.bottleneck, spec.proj, training, EPS, MOMENTUM, 0, fold_fwd,
                             self.side)
        torch.cuda.synchronize()
        for t, k in zip([x] + ws, keep):
            assert torch.equal(t.view(torch.int16), k.view(torch.int16)), "block_fwd changed an input"
        assert len(r) == 8 + 4 * spec.nbn
        c = self._c
        y = [c(r[1]), c(r[3])] + ([c(r[5])] if spec.bottleneck else []) + ([c(r[6])] if spec.proj else [])
        act = [c(r[2])] + ([c(r[4])] if spec.bottleneck else [])
        if not spec.bottleneck:
            assert c(r[4]) is None and c(r[5]) is None
        if not spec.proj:
            assert c(r[6]) is None
        st = [dict(zip(("scale", "shift", "mean", "invstd"),
                       (None if t is None or t.numel() == 0 else t.cpu() for t in r[8 + 4 * i:12 + 4 * i])))
              for i in range(spec.nbn)]
        bits = None if r[7] is None or r[7].numel() == 0 else r[7].cpu().numpy()
        return dict(out=c(r[0]), y=y, a=act, bits=bits, st=st, rm=[bn[4 * i + 2].cpu() for i in range(spec.nbn)],
                    rv=[bn[4 * i + 3].cpu() for i in range(spec.nbn)])

    def bwd(self, a):
        spec = a["spec"]
        dev = self.dev
        e = torch.empty(0, dtype=BF16, device=dev)
        ef = torch.empty(0, dtype=F32, device=dev)
        y, ins = [self._b(t) for t in a["y"]], [self._b(t) for t in a["ins"]]
        bits = torch.from_numpy(np.ascontiguousarray(a["bits"])).to(dev)
        fold = a["fold"]
        fold_w = []
        if fold:
            fold_w = [self._b(a["ws"][2 + k]) for k in range(fold["n"])]
            if fold["grams"]:
                for k in range(fold["n"]):
                    g2 = _rows(a["ins"][2 + k if k == 0 else 0])
                    Kk = g2.shape[1]
                    fold_w += [self._v((g2.t() @ g2).reshape(Kk, 1, 1, Kk)), self._v(g2.sum(0))]
        if spec.bottleneck:
            saved = [ins[0], y[0], ins[1], y[1], ins[2], e if (fold and fold["no_y3"]) else y[2],
                     y[3] if spec.proj else e, bits]
        else:
            saved = [ins[0], y[0], ins[1], y[1], e, e, y[2] if spec.proj else e, bits]
        bnst = [self._v(s[k]) for s in a["st"] for k in ("sc", "sh", "mu", "iv")]
        wt = [self._b(t) for t in a["wt"]]
        dw = [self._v(t).clone() for t in a["dw"]]
        dg, db = [self._v(t).clone() for t in a["dg"]], [self._v(t).clone() for t in a["db"]]
        bng = [t for i in range(spec.nbn) for t in (self._v(a["gamma"][i]), dg[i], db[i])]
        gam = bng[0::3]
        dout = self._b(a["dout"])
        slab = None if a["in_slab"] is None else self._v(a["in_slab"])
        prev = []
        if a["prev"] is not None:
            p = a["prev"]
            prev = [e if p["noy"] else self._b(p["ya"]), self._v(p["ma"]), self._b(p["yb"]) if p["two"] else e,
                    self._v(p["mb"]) if p["two"] else ef, torch.from_numpy(np.ascontiguousarray(p["bits"])).to(dev)]
            if p["masked"]:
                prev.append(torch.ones(1, dtype=torch.uint8, device=dev))
        noy = bool(fold and fold["no_y3"])
        # the one input block_bwd may write: the last two rows of in_slab of a forward-folded block
        slab_in = [] if slab is None else [slab[:slab.shape[0] - 2] if noy else slab]
        inputs = [dout] + saved + bnst + wt + gam + slab_in + prev + fold_w
        keep = [t.clone() for t in inputs]
        dx, pslab = self.m.block_bwd(dout, saved, bnst, wt, dw, bng, spec.stride, spec.bottleneck, spec.proj, self.side,
                                     0, slab, prev, fold_w)
        if self.side:
            torch.cuda.synchronize()
            self.m.side_stash_release()
        torch.cuda.synchronize()
        for t, k in zip(inputs, keep):
            assert torch.equal(t.reshape(-1).view(torch.uint8), k.reshape(-1).view(torch.uint8)), \
                "block_bwd changed an input"
        return dict(dx=dx.cpu().to(F64), prev_slab=None if pslab is None or pslab.numel() == 0 else pslab.cpu(),
                    dw=[t.cpu() for t in dw], dg=[t.cpu() for t in dg], db=[t.cpu() for t in db],
                    in_slab=None if slab is None else slab.cpu())


# ---------------------------------------------------------------- comparison ------------------

def interval(ref, delta):
    """The bf16 values a correctly rounded store of ref ± delta can take: (lo, hi)."""
    return rne_bf16(f32_down(ref - delta)), rne_bf16(f32_up(ref + delta))


def between(stats, name, got, lo, hi, ref, delta, ctx="", scale=1.0, reach=0.0):
    """lo <= got <= hi; records |got − ref| / (δ + reach + half a bf16 ulp of the larger end).
    ``reach``: what earlier roundings of the chain can move the value by themselves. ``scale`` < 1
    narrows δ (not the roundings) for the twin's half-bound test."""
    got = got.to(F64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite result {ctx}"
    half = torch.maximum(lo.abs(), hi.abs()) * U8
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (delta + reach + half))
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), ratio.max().item())
    bad = (got < lo) | (got > hi) | (err > scale * delta + reach + half)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name} {ctx}: {int(bad.sum())} of {bad.numel()} values outside the bf16 interval, "
                             f"first at {i}: got {got[i].item()!r}, interval [{lo[i].item()!r}, {hi[i].item()!r}], "
                             f"ref {ref[i].item()!r}")


def check_store(stats, name, got, ref, mag, kdim, ctx=""):
    delta = gamma(kdim) * mag
    lo, hi = interval(ref, delta)
    between(stats, name, got, lo, hi, ref, delta, ctx)


def stat_carry(ref, count, dS1, dS2, g, mom):
    """The error of a finalize's results caused by errors dS1, dS2 of its sums (docstring)."""
    n = float(count)
    mean, inv = ref["mean"], ref["invstd"]
    var = 1.0 / (inv * inv) - float(np.float32(EPS))
    dmean = dS1 / n
    dvar = dS2 / n + 2 * mean.abs() * dmean + dmean * dmean
    low = (var - dvar + float(np.float32(EPS))).clamp_min(1e-30)
    dinv = dvar / (2 * low ** 1.5)
    gm = g.to(F64).abs()
    return dict(mean=dmean, invstd=dinv, scale=gm * dinv, shift=gm * (mean.abs() * dinv + inv * dmean + dmean * dinv),
                running_mean=mom * dmean, running_var=mom * dvar * n / max(n - 1.0, 1.0))


def check_forward(impl, kind, shape, mode, stats=None, scale=1.0):
    """Every slot block_fwd returns against one oracle stage fed the returned slots."""
    a = fwd_inputs(kind, shape)
    spec, N, H, W, P, Q = geometry(kind, shape)
    training, fold_fwd = mode != "eval", mode == "train_fold_fwd"
    ctx = f"({kind}, {shape}, {mode})"
    got = impl.fwd(a, training, fold_fwd)
    L, n = spec.nconv - 1, spec.nconv
    folded = fold_fwd and spec.bottleneck
    assert len(got["a"]) == L and all(t is not None for t in got["a"]), f"activation slots {ctx}"
    ins = [a["x"]] + list(got["a"]) + ([a["x"]] if spec.proj else [])      # conv i reads ins[i]
    s3 = None
    for i, (K, R, Cc, s, p) in enumerate(spec.convs):
        cs = O.conv_stage(ins[i], a["ws"][i], s, p)
        kdim = R * R * Cc
        delta = gamma(kdim) * cs["mag"]
        name = f"y{i + 1}" if i < n else "ys"
        if folded and i == L:
            assert got["y"][i] is None, f"fold_fwd: y3 must be undefined {ctx}"
            s3 = (cs["s"], delta)
        else:
            assert got["y"][i] is not None, f"{name} missing {ctx}"
            lo, hi = interval(cs["s"], delta)
            between(stats, "conv store", got["y"][i], lo, hi, cs["s"], delta, f"{name} {ctx}", scale)
        g, b, rm, rv = a["bns"][4 * i:4 * i + 4]
        st = got["st"][i]
        if training:
            count = spec.bn_rows(i, N, H, W)
            rows = cs["s"].numel() // K
            assert count == rows
            sa = _rows(cs["s"]).abs()
            dl = _rows(delta)
            dS1 = dl.sum(0) + gamma(rows + 2) * sa.sum(0)
            dS2 = (2 * sa * dl + dl * dl).sum(0) + gamma(rows + 3) * (sa * sa).sum(0)
            ref = O.bn_stage(cs["sums"], count, g, b, EPS, MOMENTUM, rm, rv)
            carry = stat_carry(ref, count, dS1, dS2, g, MOMENTUM)
            fb = BC.finalize_bounds(ref)
            res = dict(st, running_mean=got["rm"][i], running_var=got["rv"][i])
            for k in fb:
                within(stats, f"bn {k}", res[k], ref[k], (fb[k] + carry[k] * (1 + 4 * U24)) * scale, ctx=f"bn{i + 1} {ctx}")
        else:
            rsc, rsh = O.eval_stage(g, b, rm, rv, EPS)
            terms = b.to(F64).abs() + (rsh - b.to(F64)).abs()
            within(stats, "eval scale", st["scale"], rsc, BC.EVAL_AFFINE_TOL * rsc.abs(), ctx=f"bn{i + 1} {ctx}")
            within(stats, "eval shift", st["shift"], rsh, BC.EVAL_AFFINE_TOL * terms, ctx=f"bn{i + 1} {ctx}")
            assert st["mean"] is None and st["invstd"] is None, f"eval: batch statistics returned {ctx}"
            BC.same_bits("eval running_mean", got["rm"][i], rm, ctx)
            BC.same_bits("eval running_var", got["rv"][i], rv, ctx)
        if i < L:
            z, T = O.act_stage(got["y"][i], st["scale"], st["shift"])
            within(stats, "bn_apply act", got["a"][i], z, U8 * z.abs() + U22 * T * scale, ctx=f"a{i + 1} {ctx}")
    stL = got["st"][L]
    if spec.proj:
        res = (got["y"][n], got["st"][n]["scale"], got["st"][n]["shift"], 1)
    else:
        res = (a["x"], None, None, 2)
    if folded:
        lo3, hi3 = interval(*s3)
        y3r = rne_bf16(s3[0].to(F32).to(F64))
        z, T = O.act_stage(y3r, stL["scale"], stL["shift"], *res)
        extra = (1 + U8 + U22) * stL["scale"].to(F64).abs() * torch.maximum(hi3 - y3r, y3r - lo3)
    else:
        z, T = O.act_stage(got["y"][L], stL["scale"], stL["shift"], *res)
        extra = 0.0
    within(stats, "bn_apply out", got["out"], z, U8 * z.abs() + U22 * T * scale + extra, ctx=ctx)
    if training:
        assert got["bits"] is not None
        assert np.array_equal(np.asarray(got["bits"]).reshape(-1), B.relu_bits(got["out"])), \
            f"the output bitmask is not out > 0 of the returned out {ctx}"
    else:
        assert got["bits"] is None, f"eval: a mask was returned {ctx}"
    return got


def _apply_bound(z, T, pert, scale=1.0):
    """u8·(|z| + pert) + u22·(T + pert) + pert; ``scale`` narrows the fp32 arithmetic's allowance,
    not the reach of a rounding (u8·|z| is the bf16 rounding's own at a power of two, and pert
    carries the roundings of the stage before)."""
    return U8 * (z.abs() + pert) + pert + scale * U22 * (T + pert)


def _sink_rest(stats, spec, i, a, got, dy, N, H, W, ctx):
    """Every sink entry against sink + wgrad(transcript): the transcript entries are the copy
    itself, the rest checks ``+=`` (non-zero pre-fill)."""
    K, R, Cc, s, p = spec.convs[i]
    ref, mag = O.wgrad_stage(dy, a["ins"][i], R, s, p)
    before = a["dw"][i].to(F64)
    within(stats, "dW sink", got["dw"][i], before + ref, 2 * U24 * (before.abs() + mag), ctx=f"conv {i} {ctx}")


def fold_dgrad_ref(c, b, dz, src, W, mu, cat=True):
    """The folded data gradient of a 1x1 conv with forward weights W [C][K] over its input
    ``src`` [rows][K] and dz [rows][C]: the unfolded fp64 value dy·W, dy = A·dz + D·(src·Wᵀ) + E,
    and the fold's own error δ (module docstring, "folded dgrad"). c / b: the oracle's
    coefficients and their bounds."""
    Cn, K = W.shape
    A, D, E = c["A"], c["D"], c["E"]
    rows = src.shape[0]
    y = src @ W.t()
    ref = (A * dz + D * y + E) @ W
    Wa, AW = W.abs(), (A[:, None] * W).abs()
    cf = torch.stack([A, D, E])
    mx, mxabs = BO.prep_mx(cf, W)
    eta = U8 * mx.abs() + (1 + U8) * gamma(FC.mx_depth(Cn, K)) * mxabs           # [l][k]
    m1 = BO.mean_dz(cf, mu, Cn).abs()
    mean_a = src.abs().sum(0) / rows
    u = U8 + 8 * U24
    err_wd = u * ((dz.abs() + m1) @ AW)
    err_mx = (src.abs() + mean_a) @ eta.t()
    bterms = E.abs() @ Wa + u * (m1 @ AW) + eta @ mean_a
    err_b = gamma(FC.bias_depth(Cn, K)) * bterms + U24 * (m1 @ AW)
    err_c = (b["A"] * dz.abs() + b["D"] * y.abs() + b["E"]) @ Wa
    mag = dz.abs() @ AW + src.abs() @ (mx.abs() + eta).t() + bterms
    err_t = 0.0
    if not cat:
        # T = bf16(src·Mx + b) is stored before it joins the accumulators: one more bf16 rounding,
        # of |T| <= |src·Mx + Eᵀ·W| + the correction terms of b + what T's own GEMM errs by
        t_abs = (src @ mx.t() + E @ W).abs() + u * (m1 @ AW) + eta @ mean_a + err_mx + err_b
        err_t = U8 * (t_abs + gamma(K + 2) * mag) + U24 * t_abs
    return ref, err_wd + err_mx + err_b + err_c + err_t + gamma(Cn + K + 2) * mag


def _fold_wgrad_check(stats, a, got, i, c, b, dz, src, W, ctx):
    """The folded weight gradient of conv i: sink + diag(A)·G + diag(D)·W·S + E ⊗ Σsrc."""
    Cn, K = W.shape
    G, S, cs = dz.t() @ src, src.t() @ src, src.sum(0)
    before = a["dw"][i].to(F64).reshape(Cn, K)
    ref, terms = BO.wgrad(torch.stack([c["A"], c["D"], c["E"]]), G, S, cs[None], W, before)
    pert = b["A"][:, None] * G.abs() + b["D"][:, None] * (W.abs() @ S.abs()) + b["E"][:, None] * cs.abs()[None, :]
    within(stats, "folded dW", got["dw"][i].to(F64).reshape(Cn, K), ref, gamma(K + 5) * terms + pert * (1 + U22),
           ctx=f"conv {i} {ctx}")


def check_backward(impl, kind, shape, mode, stats=None, scale=1.0):
    """Stage by stage along the transcripts; see the module docstring for each bound."""
    a = bwd_args(kind, shape, mode)
    spec, N, H, W, P, Q = geometry(kind, shape)
    ctx = f"({kind}, {shape}, {mode})"
    got = impl.bwd(a)
    L, n = spec.nconv - 1, spec.nconv
    st, y = a["st"], a["y"]
    fold = a["fold"]
    folded = ([L] + ([n] if fold["n"] == 2 else [])) if fold else []        # convs without a transcript
    if fold:
        # which form each folded dgrad takes (mirror of conv_plan.h): concatenated at the table's
        # widths, Wd + T at C3 = 3·K3
        cat3 = dgrad_cat_supported(spec.cout, spec.mid)
        assert cat3 == (kind != NONCAT_KIND) and (fold["n"] == 1 or dgrad_cat_supported(spec.cout, spec.cin))
    T = [None if i in folded else transcript(spec, i, a["dw"][i], got["dw"][i], N, H, W) for i in range(spec.nbn)]
    for i in range(spec.nbn):
        if i not in folded:
            _sink_rest(stats, spec, i, a, got, T[i], N, H, W, ctx)
    # ---- the output BN (and the shortcut BN, fed by the same dz)
    ms = None if fold else ("bits", a["bits"])          # fold: dout is dz, already masked
    cnt = N * P * Q
    two = spec.proj
    slab_sums = None
    if a["in_slab"] is not None:
        sl = a["in_slab"].to(F64)
        after = got["in_slab"]
        if fold and fold["no_y3"]:
            # bnfold_rowdot: the LAST two rows become [0, hi, 0] / [0, lo, 0] of Σdz·y3 = Σ_k W3·G,
            # every other row stays as it was
            W3 = a["ws"][2].reshape(spec.cout, spec.mid)
            v, vt = BO.rowdot(_rows(a["dout"]).t() @ _rows(a["ins"][2]), W3)
            BC.same_bits("in_slab rows before the last two", after[:-2], a["in_slab"][:-2], ctx)
            assert (after[-2:, 0] == 0).all() and (after[-2:, 2:] == 0).all(), f"extra rows: sets 0 / 2 not zero {ctx}"
            hl = after[-2:, 1].to(F64)
            within(stats, "rowdot rows", hl.sum(0), v, spec.mid * 2.0 ** -53 * vt + 2.0 ** -48 * v.abs(), ctx=ctx)
            assert (hl[1].abs() <= BO.ulp32(hl[0]) / 2).all(), f"extra rows: lo is not a remainder of hi {ctx}"
            sl = after.to(F64)
        else:
            BC.same_bits("in_slab", after, a["in_slab"], ctx)
        slab_sums = sl.sum(0)
        dS = sl.shape[0] * U52 * sl.abs().sum(0)
    r = O.bn_bwd_stage(a["dout"], ms, y[L], st[L]["mu"], st[L]["iv"], a["gamma"][L], cnt,
                       y[n] if two else None, st[n]["mu"] if two else None, st[n]["iv"] if two else None,
                       a["gamma"][n] if two else None, sums=slab_sums)
    if slab_sums is None:
        dS = (BC.reduce_n_t(cnt, spec.cout) + 3) * U24 * r["abs_sums"]
    dzabs = _rows(r["dz"]).abs()
    fold_da, fold_dxs = None, None
    for key, i, si in (("a", L, 0), ("b", n, 1))[:2 if two else 1]:
        c = r["c" + key]
        b = BC.coef_bounds(c, a["dg"][i], a["db"][i], cnt, st[i]["iv"], st[i]["mu"], 1.0, dS[0], dS[1 + si])
        within(stats, "dgamma", got["dg"][i], c["dgamma"] + a["dg"][i].to(F64), b["dgamma"], ctx=f"bn {i} {ctx}")
        within(stats, "dbeta", got["db"][i], c["dbeta"] + a["db"][i].to(F64), b["dbeta"], ctx=f"bn {i} {ctx}")
        if i in folded:
            Wi = a["ws"][i].reshape(spec.convs[i][0], spec.convs[i][2])
            src = _rows(a["ins"][i])
            _fold_wgrad_check(stats, a, got, i, c, b, _rows(a["dout"]), src, Wi, ctx)
            ref, dl = fold_dgrad_ref(c, b, _rows(a["dout"]), src, Wi, st[i]["mu"].to(F64), cat3 if i == L else True)
            shp = a["ins"][i].shape
            if i == L:
                fold_da = (ref.reshape(shp), dl.reshape(shp))
            else:
                fold_dxs = (ref.reshape(shp), dl.reshape(shp))
            continue
        pert = (b["A"] * dzabs + b["D"] * _rows(y[i]).abs() + b["E"]).reshape(a["dout"].shape)
        within(stats, "dy of the output BN", T[i], r["dy" + key], _apply_bound(r["dy" + key], r["T" + key], pert, scale),
               ctx=f"bn {i} {ctx}")
    # ---- dgrad -> block-internal BN, twice for a bottleneck
    for i in range(L, 0, -1):
        K, R, Cc, s, p = spec.convs[i]
        j = i - 1
        h, w = a["ins"][i].shape[1], a["ins"][i].shape[2]
        if i == L and fold:
            acc, delta = fold_da
        else:
            acc, mag = O.dgrad_stage(T[i], a["wt"][i], h, w, s, p)
            delta = gamma(R * R * K) * mag
        dda = delta + U8 * (acc.abs() + delta)
        rows = spec.bn_rows(j, N, H, W)
        assert rows == acc.numel() // acc.shape[-1]
        mj = ("affine", st[j]["sc"], st[j]["sh"])
        rj = O.bn_bwd_stage(acc, mj, y[j], st[j]["mu"], st[j]["iv"], a["gamma"][j], rows)
        m = (_rows(y[j]) * st[j]["sc"].to(F64) + st[j]["sh"].to(F64) > 0).to(F64)
        da_m, dda_m = _rows(acc).abs() * m, _rows(dda) * m
        ymu = (_rows(y[j]) - st[j]["mu"].to(F64)).abs()
        g3 = gamma(rows + 3)
        dS0 = dda_m.sum(0) + g3 * (da_m + dda_m).sum(0)
        dS1 = (dda_m * ymu).sum(0) + g3 * ((da_m + dda_m) * ymu).sum(0)
        c = rj["ca"]
        b = BC.coef_bounds(c, a["dg"][j], a["db"][j], rows, st[j]["iv"], st[j]["mu"], 1.0, dS0, dS1)
        within(stats, "dgamma (internal)", got["dg"][j], c["dgamma"] + a["dg"][j].to(F64), b["dgamma"],
               ctx=f"bn {j} {ctx}")
        within(stats, "dbeta (internal)", got["db"][j], c["dbeta"] + a["db"][j].to(F64), b["dbeta"],
               ctx=f"bn {j} {ctx}")
        pert = ((c["A"].abs() + b["A"]) * dda_m + b["A"] * da_m + b["D"] * _rows(y[j]).abs() + b["E"]).reshape(acc.shape)
        within(stats, "dy of an internal BN", T[j], rj["dya"], _apply_bound(rj["dya"], rj["Ta"], pert, scale),
               ctx=f"bn {j} {ctx}")
    # ---- the final dgrad: dx = bf16(bf16(acc1) + addend)
    K, R, Cc, s, p = spec.convs[0]
    acc1, mag1 = O.dgrad_stage(T[0], a["wt"][0], H, W, s, p)
    d1 = gamma(R * R * K) * mag1
    lo1, hi1 = interval(acc1, d1)
    if fold_dxs is not None:
        accs, ds = fold_dxs
        los, his = interval(accs, ds)
    elif spec.proj:
        if spec.stride > 1:
            accs, mags = O.dgrad_stage(T[n], a["wt"][n], P, Q, 1, 0)
            place = lambda t: O.subgrid(t, spec.stride, H, W)
        else:
            accs, mags = O.dgrad_stage(T[n], a["wt"][n], H, W, 1, 0)
            place = lambda t: t
        ds = gamma(spec.cout) * mags
        los, his = interval(accs, ds)
        los, his, accs, ds = place(los), place(his), place(accs), place(ds)
    else:
        add = a["dout"] if fold else a["dout"] * C.unpack_bits(a["bits"], a["dout"].shape)
        los, his, accs, ds = add, add, add, torch.zeros_like(add)
    lo, hi = rne_bf16(f32_down(lo1 + los)), rne_bf16(f32_up(hi1 + his))
    half1 = torch.maximum(lo1.abs(), hi1.abs()) * U8
    dx_ref, dx_delta = acc1 + accs, d1 + ds
    dx_reach = half1 + torch.maximum(los.abs(), his.abs()) * U8 * (ds > 0)
    dx = got["dx"]
    if a["prev"] is not None:
        pv = a["prev"]
        if pv["masked"]:
            # the unmasked dx of a second call, times the mask, bit for bit
            plain = impl.bwd(bwd_args(kind, shape, "prev2" if pv["two"] else "prev1"))["dx"]
            mk = C.unpack_bits(pv["bits"], plain.shape) > 0
            # kept elements bit for bit; a dropped element is a zero (of either sign: dx·0 and a
            # select differ there, and both are "dx times the mask")
            kept = np.array_equal(B.bf16_bits(dx[mk]), B.bf16_bits(plain[mk]))
            nz = int((dx[~mk] != 0).sum())
            assert kept and nz == 0, f"masked store != dx·mask {ctx}: kept elements bit-equal: {kept}, " \
                                     f"{nz} of {int((~mk).sum())} dropped elements are not zero"
            dx = plain
        # the slab: sums of the stored (unmasked) dx under the previous block's mask
        d, terms = C.bn_terms(dx, ("bits", pv["bits"]), None if pv["noy"] else pv["ya"], pv["ma"],
                              pv["yb"] if pv["two"] else None, pv["mb"] if pv["two"] else None)
        slab = got["prev_slab"]
        assert slab is not None, f"no prev_slab {ctx}"
        ex = 2 if pv["noy"] else 0
        assert slab.dim() == 3 and slab.shape[0] > ex and slab.shape[1] == terms.shape[0] and slab.shape[2] == spec.cin, \
            f"prev_slab shape {tuple(slab.shape)} {ctx}"
        if pv["noy"]:
            # placement: the two rows left for the caller come LAST. The executor guarantees nothing
            # about their content (conv_dgrad_bnstat allocates the slab uninitialised and its kernel
            # never touches them); the previous block's bnfold_rowdot writes every set of both rows
            # before anything reads them, which the no_y3 mode checks. The rows before them are the
            # masked-store call's rows (set 0, Σdz, does not depend on the missing y3)
            ms_slab = impl.bwd(bwd_args(kind, shape, "prev_masked"))["prev_slab"]
            assert slab.shape[0] == ms_slab.shape[0] + 2, f"prev_slab rows {slab.shape[0]} != {ms_slab.shape[0]} + 2 {ctx}"
            BC.same_bits("prev_slab set 0 row by row", slab[:-2, 0].contiguous(), ms_slab[:, 0].contiguous(), ctx)
        sums = slab[:slab.shape[0] - ex].to(F64).sum(0)
        within(stats, "prev_slab", sums, terms.sum(1), gamma(N * H * W + 3) * terms.abs().sum(1) * scale, ctx=ctx)
    else:
        assert got["prev_slab"] is None, f"a prev_slab without prev {ctx}"
    between(stats, "dx", dx, lo, hi, dx_ref, dx_delta, ctx, scale, dx_reach)
    return got


# ---------------------------------------------------------------- defects ---------------------
# defect -> ("fwd" | "bwd", kind, shape, mode): the case at which it must fail
DEFECT_CASES = {
    "proj_bn_input_rows": ("fwd", "bott_proj_s2", "3x3x3", "train"),
    "residual_after_relu": ("fwd", "bott_id", "2x4x4", "train"),
    "mask_before_residual": ("fwd", "basic_id", "2x4x4", "train"),
    "dbeta3_to_shortcut_sink": ("bwd", "bott_proj_s1", "2x4x4", "noslab"),
    "biased_running_var": ("fwd", "basic_id", "3x3x3", "train"),
    "momentum_on_old": ("fwd", "basic_id", "3x3x3", "train"),
    "dgamma_overwritten": ("bwd", "basic_id", "2x4x4", "noslab"),
    "subgrid_offset_1_1": ("bwd", "basic_proj_s2", "3x3x3", "noslab"),
    "shortcut_dx_dropped": ("bwd", "bott_proj_s2", "2x4x4", "noslab"),
    "store_masked_ignored": ("bwd", "bott_id", "2x4x4", "prev_masked"),
    "bn2_mean_for_bn1": ("bwd", "bott_id", "3x3x3", "noslab"),
    "eval_batch_stats": ("fwd", "bott_proj_s1", "2x4x4", "eval"),
    "third_slab_set_missing": ("bwd", "bott_proj_s2", "3x3x3", "prev2"),
    "extra_rows_first": ("bwd", "bott_id", "2x4x4", "no_y3"),
    "fold_E_missing": ("bwd", "bott_id", "3x3x3", "fold"),
    "fold_gram_of_x": ("bwd", "bott_proj_s2", "2x4x4", "fold"),
}


def run_case(impl, direction, kind, shape, mode, stats=None, scale=1.0):
    return (check_forward if direction == "fwd" else check_backward)(impl, kind, shape, mode, stats, scale)
