"""Cases, bounds and implementations of the contrastive-loss oracle tests (csrc/kernels/supcon.hip).

An *implementation* has three methods on CPU tensors: ``fwd`` -> dict(loss, lse, invcnt, rows),
``bwd`` -> (dA, dC) and ``bwd_sum`` -> dX. ``ExtImpl`` runs the HIP kernels, ``TwinImpl`` a CPU
fp32 twin of the kernel's arithmetic (optionally with one deliberate defect from ``WRONG``).
tests/test_supcon_oracle.py holds the twin to the bounds on the CPU (ratio <= 0.5 in two
accumulation orders) and shows every defect outside them (> 4x) at the cases ``WRONG`` names;
tests/test_gpu_supcon_oracle.py holds the kernels to the same bounds.

Bounds of the kernel against ``supcon_oracle.split_model`` (u = 2^-24, first order in u, times
SECOND_ORDER for the products of roundings). Only fp32 accumulation and the fast intrinsics
separate the two:

  logit     E_ij = u·(1 + 2^-7)/τ·Σ_d W_d|a_d||c_d| + 3u·|s_ij|
            The 3·D products of bf16 values are exact in fp32. They are added by n_chain = 3·D/32
            chained MFMAs of 32 products each, the accumulator being one more operand of each.
            The order inside one MFMA is not documented, so every operand of an MFMA, the incoming
            accumulator included, is charged its 32 additions: a hi·hi product of k-step
            s = d // 32 enters at chain position 3s + 1 and sees W_d = 32·(n_chain − 3s)
            roundings; the hi·lo and lo·hi products are at most 2^-8 of it and see fewer
            ((1 + 2^-7) covers |hi| <= (1 + 2^-9)|x| and both). 3u·|s|: (float)(1/τ) and the product.
  exp       __expf(x) = exp(x)·(1 + δ), |δ| <= K_EXP·(1 + |x|)·u; __logf(l) = log(l) + ε,
            |ε| <= K_LOG·(1 + |log l|)·u. Neither the guides nor the ROCm headers on hand state
            the error of these intrinsics, so this is the model the issue prescribes: the argument
            is multiplied by log2(e) in fp32 (a relative u·|x·log2e|, i.e. u·|x| absolute in the
            exponent, twice: the constant and the product) and v_exp_f32 / v_log_f32 are taken as
            good to about one ulp (2u). K_EXP = K_LOG = 4; the twin (exp2 of an explicit fp32
            product with log2(e)) measures 0.03 of the lse bound and 0.02 of the row-loss
            bound at most with these (0.38 of the dC bound, where exp enters through G).
  lse       every term exp(s_ij − m_i) of l_i passes through a chain of exp factors whose
            arguments are all <= 0 and sum to x_ij = s_ij − m_i: its own exp and one rescale per
            later tile, per shuffle step (2) and per split of the finalize combine: R factors and
            R products; and through at most n_add fp32 additions. All terms are positive, so
            the relative error of l_i is the softmax-weighted mean of the per-term ones:
              B_l = u·(K_EXP·(R + Σ_j p_ij|x_ij|) + R + n_add)
            lse is 1-Lipschitz in the logits in the max norm:
              B_lse = max_j E_ij + B_l + K_LOG·u·(1 + |log l_i|) + u·|lse_i|
  invcnt    the count is an exact fp32 integer: |got − 1/cnt| <= 2u/cnt (division within an
            ulp); exactly −1 without positives
  row loss  B_row = (τ/τ_base)·(mean_pos E + (n_add + 1)·u·mean_pos|s| + B_lse + u·|mean − lse|) + 2u·|ℓ|
            exactly 0 without positives
  loss      B_loss = |scale|·(Σ B_row + n_sum·u·Σ|ℓ|) + 2u·|loss|, n_sum = ceil(Na/1024) + 22
            (per-thread stride loop, 6 shuffle steps, 16 wave partials)
  gradient  the backward is given the implementation's own lse and invcnt.
            ΔG_ij <= |w·g|·(p_ij·(E_ij + B_lse_i + (K_EXP + 1)·u·(1 + |log p_ij|)) + 2u·pos_ij/cnt) + 3u·|G_ij|
            three-term truncation, kernel and model each on its own G: 2·ε₃·|G_ij||c_j|,
              ε₃ = 3·2^-18·(1 + 2^-7)  (lo·lo and the two remainders of the splits)
            accumulation: 3 MFMAs of 32 products per tile, worst order as above, then the slab
            sum: n3 = 96·tiles_per_split + n_slabs roundings
              B_dA = Σ_j (ΔG_ij + (2ε₃ + n3·u)·|G_ij|)·|c_j|      (dC: over i with |a_i|)
            bwd_sum: B_dA + B_dC with n_slabs = both passes' slabs.
            Rows of G without positives are exactly 0, so their contribution to the bound is 0.

``split_model`` against ``exact`` (CPU only): ``supcon_oracle.split_bound`` per logit.
"""
from __future__ import annotations

import math

import torch

import supcon_oracle as O

F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24
K_EXP = 4.0
K_LOG = 4.0
EPS3 = 3.0 * 2.0 ** -18 * (1.0 + 2.0 ** -7)
SECOND_ORDER = 1.01
TAU_BASE = 0.07

# ---------------------------------------------------------------- mirrors of the split rules ---
OTHER_TILE = 32
OWN_PER_WG = 64


def pick_splits(n_own, n_other):
    """supcon.hip pick_splits: ~512 workgroups, at least two other tiles per split."""
    own_blocks = (n_own + OWN_PER_WG - 1) // OWN_PER_WG
    s = (512 + own_blocks - 1) // own_blocks
    return max(1, min(s, (n_other + 2 * OTHER_TILE - 1) // (2 * OTHER_TILE)))


def _round_tile(n):
    return (n + OTHER_TILE - 1) // OTHER_TILE * OTHER_TILE


def fwd_geometry(n_own, n_other):
    """launch_supcon_fwd: -> (n_split, other_per_split); the split count is not recomputed after
    the rounding, so trailing splits can be empty."""
    ns = pick_splits(n_own, n_other)
    return ns, _round_tile((n_other + ns - 1) // ns)


def bwd_geometry(n_own, n_other):
    """supcon.hip bwd_splits: -> (n_split, other_per_split) with the count recomputed."""
    ns = pick_splits(n_own, n_other)
    per = _round_tile((n_other + ns - 1) // ns)
    return (n_other + per - 1) // per, per


def fwd_split_ranges(n_own, n_other):
    ns, per = fwd_geometry(n_own, n_other)
    return [(s * per, max(s * per, min((s + 1) * per, n_other))) for s in range(ns)]


def empty_fwd_splits(n_own, n_other):
    return sum(1 for a, b in fwd_split_ranges(n_own, n_other) if a >= b)


def last_tile_rows(n_own, n_other):
    """Rows of the last tile of the last non-empty forward split."""
    a, b = [r for r in fwd_split_ranges(n_own, n_other) if r[0] < r[1]][-1]
    return (b - a - 1) % OTHER_TILE + 1


# ---------------------------------------------------------------- cases ------------------------

class Case:
    def __init__(self, name, A, C, self_idx, akey, ckey, tau, g=1.7, same=False):
        self.name, self.tau, self.g, self.same = name, tau, g, same
        self.A, self.C = A.to(F32).contiguous(), C.to(F32).contiguous()
        self.self_idx, self.akey, self.ckey = (t.to(torch.int32).contiguous() for t in (self_idx, akey, ckey))
        self.Na, self.N, self.D = A.shape[0], C.shape[0], A.shape[1]
        self.scale = 1.0 / self.Na
        assert self.N >= 2 and 0 <= int(self.self_idx.min()) and int(self.self_idx.max()) < self.N
        assert not same or (self.Na == self.N and torch.equal(self.A, self.C))

    def args(self):
        return (self.A, self.C, self.self_idx, self.akey, self.ckey, self.tau, TAU_BASE, self.scale)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_rows(n, D, kind, seed):
    """Unit rows: random, or clustered (8 centres + 0.05·noise, renormalised)."""
    g = _gen(seed)
    if kind == "random":
        x = torch.randn(n, D, generator=g)
    else:
        centres = torch.nn.functional.normalize(torch.randn(8, D, generator=g), dim=1)
        x = centres[torch.randint(0, 8, (n,), generator=g)] + 0.05 * torch.randn(n, D, generator=g)
    return torch.nn.functional.normalize(x, dim=1)


def _edge(na, n, D, tau, kind, seed, same=None):
    C = make_rows(n, D, kind, seed)
    key = torch.arange(n) % 7
    si = torch.arange(na)
    same = (na == n) if same is None else same
    return Case(f"edge_{na}x{n}_D{D}", C if same else C[:na], C, si, key[:na], key, tau, same=same)


def _ownership(r, mode, method, D, tau, seed):
    """N = 384 gathered rows of W = 4 ranks; the index builder is the production one."""
    from simclr_pytorch_distributed_amd.losses.supcon import DistributedContrastiveLoss
    w, nv, b = 4, 2, 48
    crit = DistributedContrastiveLoss(method, tau, TAU_BASE, contrast_mode=mode, n_views=nv, backend="torch")
    labels_all = torch.randint(0, 5, (w * b,), generator=_gen(seed + 1)) if method == "SupCon" else None
    si, ak, ck = crit._indices(b, w, r, torch.device("cpu"), labels_all)
    C = make_rows(w * nv * b, D, "clustered", seed)
    return Case(f"own_r{r}_{mode}_{method}", C[si.long()], C, si, ak, ck, tau)


def _views(nv, n, D, tau, seed):
    C = make_rows(nv * n, D, "clustered", seed)
    key = torch.arange(n).repeat(nv)
    return Case(f"views{nv}", C, C, torch.arange(nv * n), key, key, tau, same=True)


def _max_order(name, n, row, D, tau, seed, dup_rows=()):
    """Random unit rows; contrast ``row`` is nearly equal to anchor 0 (the largest logit of its
    row by far), ``dup_rows`` are exact copies of anchor 0 at non-self rows."""
    g = _gen(seed)
    C = make_rows(n, D, "random", seed)
    if row is not None:
        C[row] = torch.nn.functional.normalize(C[0] + 0.01 * torch.randn(D, generator=g), dim=0)
    for j in dup_rows:
        C[j] = C[0]
    key = torch.arange(n) % 6
    return Case(name, C[:4].clone(), C, torch.arange(4), key[:4], key, tau)


def _build_cases():
    cs = [
        _edge(1, 33, 64, 0.5, "random", 1),
        _edge(15, 65, 128, 0.1, "clustered", 2),
        _edge(65, 65, 256, 0.07, "clustered", 3),
        _edge(64, 64, 64, 0.07, "clustered", 4),
        _edge(200, 200, 128, 0.5, "random", 5),
        _edge(129, 257, 64, 0.1, "clustered", 6),
        _edge(128, 128, 128, 0.02, "clustered", 7),       # the stress temperature
        _edge(96, 96, 256, 0.5, "random", 8),
        _edge(1500, 1500, 128, 0.07, "clustered", 9),     # 22 forward splits, 6 of them empty
    ]
    cs[6].name = "stress_tau"
    cs[8].name = "empty_splits"
    # empty splits with every logit below −88: a (0, 0) partial in place of (−inf, 0) would move
    # the maximum to 0 and flush every term of the sum (one tight cluster, rows scaled by 1.5)
    g = _gen(10)
    base = torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)
    C = 1.5 * torch.nn.functional.normalize(base + 0.02 * torch.randn(1500, 64, generator=g), dim=1)
    key = torch.arange(1500) % 7
    cs.append(Case("empty_splits_low", -C, C, torch.arange(1500), key, key, 0.02))
    # row ownership
    k = 0
    for mode in ("all", "one"):
        for method in ("SimCLR", "SupCon"):
            for r in (0, 2, 3):
                cs.append(_ownership(r, mode, method, (64, 128, 256)[k % 3], (0.5, 0.1, 0.07)[(k // 3) % 3], 20 + k))
                k += 1
    # self placement: N = 200 is four forward splits [0,64) [64,128) [128,192) [192,200)
    C = make_rows(200, 128, "clustered", 40)
    si = torch.tensor([0, 31, 32, 63, 127, 199, 192, 100])
    key = torch.arange(200) % 9
    cs.append(Case("self_place", C[si], C, si, key[si], key, 0.1))
    C = make_rows(96, 64, "clustered", 41)
    si = torch.randperm(96, generator=_gen(42))
    key = torch.arange(96) % 5
    cs.append(Case("self_perm", C[si], C, si, key[si], key, 0.07))
    # no positives
    C = make_rows(70, 128, "clustered", 43)
    key = torch.cat([torch.arange(10), 10 + torch.randint(0, 5, (60,), generator=_gen(44))])
    cs.append(Case("nopos_some", C, C, torch.arange(70), key, key, 0.1, same=True))
    C = make_rows(65, 64, "clustered", 45)
    cs.append(Case("nopos_all", C, C, torch.arange(65), torch.arange(65), torch.arange(65), 0.07, same=True))
    C = make_rows(80, 256, "clustered", 46)
    key = torch.arange(40).repeat(2)
    key[40 + 17] = 9999
    cs.append(Case("nopos_one", C[:40], C, torch.arange(40), key[:40], key, 0.07))
    cs += [_views(3, 22, 64, 0.1, 47), _views(4, 17, 128, 0.07, 48)]
    C = make_rows(72, 256, "clustered", 49)                # n_views = 1 where every label has a partner
    key = torch.arange(72) % 9
    cs.append(Case("views1", C, C, torch.arange(72), key, key, 0.5, same=True))
    # the position of the maximum. N = 96: forward splits [0,64) [64,96); N = 97: [0,64) [64,97)
    cs += [_max_order("max_first", 96, 5, 128, 0.07, 50), _max_order("max_last", 96, 90, 64, 0.02, 51),
           _max_order("max_tail", 97, 96, 256, 0.07, 52), _max_order("dup", 97, None, 128, 0.07, 53, (10, 50, 96))]
    # upstream gradient
    for name, gv in (("g_zero", 0.0), ("g_neg", -0.6)):
        c = _edge(64, 64, 128, 0.1, "clustered", 54)
        c.name, c.g = name, gv
        cs.append(c)
    assert len({c.name for c in cs}) == len(cs)
    return cs


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = {c.name: c for c in _build_cases()}
    return _cases


def case_names():
    return list(cases())


REPEAT_CASES = ["empty_splits", "own_r2_all_SimCLR"]


def path_facts(c):
    """What the split mirrors say about a case (tests/test_supcon_oracle.py asserts the named ones)."""
    ranges = fwd_split_ranges(c.Na, c.N)
    si = c.self_idx.long().tolist()
    live = [(a, b) for a, b in ranges if a < b]
    return dict(fwd_splits=len(ranges), empty=empty_fwd_splits(c.Na, c.N), bwd_a=bwd_geometry(c.Na, c.N)[0],
                bwd_c=bwd_geometry(c.N, c.Na)[0], last_tile=last_tile_rows(c.Na, c.N),
                self_first_of_tile=sum(1 for s in si if s % OTHER_TILE == 0),
                self_last_of_tile=sum(1 for s in si if s % OTHER_TILE == OTHER_TILE - 1),
                self_last_of_split=sum(1 for s in si if any(s == b - 1 for _, b in live)),
                self_last_row=sum(1 for s in si if s == c.N - 1),
                self_alone_in_split=sum(1 for s in si if any(a == s and b == s + 1 for a, b in live)),
                no_pos=int((~_model(c)["has"]).sum()))


# ---------------------------------------------------------------- reference and bounds ----------

_models = {}


def _model(c):
    if c.name not in _models:
        M = O.split_model(*c.args(), c.g)
        M.update(_bounds(c, M))
        for k in ("P", "posw", "logits", "not_self", "pos"):      # large, no longer needed
            M.pop(k)
        _models[c.name] = M
    return _models[c.name]


def _bounds(c, M):
    u, tau, D = U24, c.tau, c.D
    zero = torch.zeros((), dtype=F64)
    absA, absC = c.A.to(F64).abs(), c.C.to(F64).abs()
    S, ns_mask, pos, P, has = M["logits"], M["not_self"], M["pos"], M["P"], M["has"]
    n_chain = 3 * D // 32
    W = (32 * (n_chain - 3 * (torch.arange(D) // 32))).to(F64)
    E = (u * (1 + 2.0 ** -7) / tau) * ((absA * W) @ absC.t()) + 3 * u * S.abs()
    # forward
    ns, per = fwd_geometry(c.Na, c.N)
    tps = per // OTHER_TILE
    R = tps + 2 + ns + 1
    n_add = 8 * tps + 2 + ns
    x = torch.where(ns_mask, (S - M["max"][:, None]).abs(), zero)
    H = (P * x).sum(1)
    B_l = u * (K_EXP * (R + H) + R + n_add)
    log_l = M["lse"] - M["max"]
    maxE = torch.where(ns_mask, E, zero).max(1).values
    B_lse = SECOND_ORDER * (maxE + B_l + K_LOG * u * (1 + log_l.abs()) + u * M["lse"].abs())
    cd = M["cnt"].clamp_min(1).to(F64)
    ratio = tau / TAU_BASE
    meanE = torch.where(pos, E, zero).sum(1) / cd
    meanS = torch.where(pos, S.abs(), zero).sum(1) / cd
    B_row = ratio * (meanE + (n_add + 1) * u * meanS + B_lse + u * (M["mean_pos"] - M["lse"]).abs()) \
        + 2 * u * M["rows"].abs()
    B_row = torch.where(has, SECOND_ORDER * B_row, zero)
    n_sum = math.ceil(c.Na / 1024) + 22
    B_loss = SECOND_ORDER * (abs(c.scale) * (B_row.sum() + n_sum * u * M["rows"].abs().sum()) + 2 * u * M["loss"].abs())
    B_ic = torch.where(has, 2 * u / cd, zero)
    # backward
    G = M["G"].abs()
    logp = torch.where(ns_mask, (S - M["lse"][:, None]).abs(), zero)
    dG = abs(M["w"] * c.g) * (P * (E + B_lse[:, None] + (K_EXP + 1) * u * (1 + logp)) + 2 * u * M["posw"]) + 3 * u * G
    dG = torch.where(has[:, None] & ns_mask, dG, zero)

    def n3(n_own, n_other, slabs=None):
        s, p = bwd_geometry(n_own, n_other)
        slabs = s if slabs is None else slabs
        return 96 * (p // OTHER_TILE) + (slabs if slabs > 1 else 0)

    def grads(n3a, n3c):
        return (SECOND_ORDER * ((dG + (2 * EPS3 + n3a * u) * G) @ absC),
                SECOND_ORDER * ((dG + (2 * EPS3 + n3c * u) * G).t() @ absA))

    B_dA, B_dC = grads(n3(c.Na, c.N), n3(c.N, c.Na))
    out = dict(B_lse=B_lse, B_rows=B_row, B_loss=B_loss, B_invcnt=B_ic, B_dA=B_dA, B_dC=B_dC)
    if c.same:
        both = 2 * bwd_geometry(c.N, c.N)[0]
        xa, xc = grads(n3(c.N, c.N, both), n3(c.N, c.N, both))
        out["B_dX"] = xa + xc
    return out


# ---------------------------------------------------------------- implementations -------------

class ExtImpl:
    """The HIP kernels of the extension module ``m`` on device ``dev``."""

    def __init__(self, m, dev):
        self.m, self.dev = m, dev

    def _d(self, *ts):
        return [t.contiguous().to(self.dev) for t in ts]

    def fwd(self, A, C, si, ak, ck, tau, tau_base, scale):
        r = self.m.supcon_fwd(*self._d(A, C, si, ak, ck), 1.0 / tau, tau / tau_base, scale)
        return dict(zip(("loss", "lse", "invcnt", "rows"), (t.cpu() for t in r)))

    def bwd(self, A, C, si, ak, ck, lse, invcnt, g, tau, tau_base, scale):
        gs = torch.tensor([g], dtype=F32, device=self.dev)
        dA, dC = self.m.supcon_bwd(*self._d(A, C, si, ak, ck, lse, invcnt), gs, 1.0 / tau,
                                   scale * (tau / tau_base) / tau)
        return dA.cpu(), dC.cpu()

    def bwd_sum(self, X, si, ak, ck, lse, invcnt, g, tau, tau_base, scale):
        gs = torch.tensor([g], dtype=F32, device=self.dev)
        return self.m.supcon_bwd_sum(*self._d(X, si, ak, ck, lse, invcnt), gs, 1.0 / tau,
                                     scale * (tau / tau_base) / tau).cpu()


WRONG = {
    # defect -> the cases at which it lies outside 4x a bound (asserted on the CPU)
    "drop_lo_hi": ["edge_64x64_D64", "edge_129x257_D64", "self_perm", "own_r0_all_SimCLR"],
    "hi_lo_twice": ["edge_64x64_D64", "edge_129x257_D64", "self_perm", "own_r0_all_SimCLR"],
    "hi_hi_only": ["edge_64x64_D64", "edge_129x257_D64", "edge_200x200_D128", "edge_65x65_D256", "empty_splits"],
    "g_hi_only": ["edge_64x64_D64", "edge_200x200_D128", "edge_65x65_D256", "own_r2_all_SimCLR"],
    "self_in_lse": ["edge_1x33_D64", "edge_64x64_D64", "self_place", "own_r3_one_SupCon"],
    "self_positive": ["edge_1x33_D64", "edge_64x64_D64", "nopos_all", "self_place"],
    "no_gate_a": ["nopos_all", "nopos_some", "nopos_one"],
    "no_gate_c": ["nopos_all", "nopos_some", "nopos_one"],
    "no_rescale": ["max_last", "max_tail", "stress_tau"],
    "empty_split_zero": ["empty_splits_low"],
    "base0_in_bwd_c": ["own_r2_all_SimCLR", "own_r3_all_SupCon", "own_r2_one_SimCLR", "self_perm"],
    "no_o_end_mask": ["edge_1x33_D64", "edge_200x200_D128", "edge_15x65_D128"],
}

_LOG2E = torch.tensor(math.log2(math.e), dtype=F32)
_LN2 = torch.tensor(math.log(2.0), dtype=F32)


def _exp(x):
    """exp as the kernel's fast intrinsic forms it: exp2 of an explicit fp32 product with log2(e)."""
    return torch.exp2(x * _LOG2E)


def _log(x):
    return torch.log2(x) * _LN2


class TwinImpl:
    """fp32 CPU twin: the hi/lo split, the three-term products, the online max/sum recurrence per
    32-row tile, per lane group (rows 4h + r and 16 + 4h + r of a tile) and per split, the shuffle
    and finalize combines and the backward with its per-split slabs, all in fp32. ``reverse``
    walks the tiles of a split and the splits in the opposite order."""

    def __init__(self, wrong=None, reverse=False):
        assert wrong is None or wrong in WRONG
        self.wrong, self.reverse = wrong, reverse

    def _order(self, seq):
        seq = list(seq)
        return seq[::-1] if self.reverse else seq

    def _prod(self, other, own):
        """S^T tile as the kernel chains it: other_hi·own_hi + other_hi·own_lo + other_lo·own_hi -> [n_own, 32]"""
        (oh, ol), (wh, wl) = other, own
        acc = wh @ oh.t()
        if self.wrong == "hi_hi_only":
            return acc
        acc = acc + wl @ oh.t()
        if self.wrong == "drop_lo_hi":
            return acc
        return acc + (wl @ oh.t() if self.wrong == "hi_lo_twice" else wh @ ol.t())

    @staticmethod
    def _tile(split_rows, ob, o_end, n_pad=OTHER_TILE):
        """Rows ob .. ob+31 of (hi, lo), zero past o_end (as the staging loop fills them)."""
        hi, lo = split_rows
        n = max(0, min(o_end - ob, n_pad))
        th, tl = torch.zeros(n_pad, hi.shape[1]), torch.zeros(n_pad, hi.shape[1])
        th[:n], tl[:n] = hi[ob:ob + n], lo[ob:ob + n]
        return th, tl

    @staticmethod
    def _pad_keys(key):
        return torch.cat([key.long(), torch.full((OTHER_TILE,), -(2 ** 40))])

    def _combine(self, m1, l1, m2, l2):
        mn = torch.maximum(m1, m2)
        l = l1 * _exp(m1 - mn) + l2 * _exp(m2 - mn)
        return mn, torch.where(mn > -math.inf, l, torch.zeros(()))

    def fwd(self, A, C, si, ak, ck, tau, tau_base, scale):
        Na, N = A.shape[0], C.shape[0]
        own, other = O.split(A), O.split(C)
        inv_temp = torch.tensor(1.0 / tau, dtype=F32)
        si, ak = si.long(), ak.long()
        ckp = self._pad_keys(ck)
        ns, per = fwd_geometry(Na, N)
        parts = []
        for s in range(ns):
            o0, o1 = s * per, min((s + 1) * per, N)
            run_m, run_l = torch.full((Na, 4), -math.inf), torch.zeros(Na, 4)
            ps, pc = torch.zeros(Na, 4), torch.zeros(Na, 4)
            for ob in self._order(range(o0, o1, OTHER_TILE)):
                rows = torch.arange(ob, ob + OTHER_TILE)
                sv = self._prod(self._tile(other, ob, o1), own) * inv_temp
                inb = torch.ones(OTHER_TILE, dtype=torch.bool) if self.wrong == "no_o_end_mask" else rows < o1
                not_self = rows[None, :] != si[:, None]
                valid = inb[None, :] & not_self
                valid_lse = inb[None, :].expand(Na, -1) if self.wrong == "self_in_lse" else valid
                valid_pos = inb[None, :].expand(Na, -1) if self.wrong == "self_positive" else valid
                ispos = valid_pos & (ckp[rows][None, :] == ak[:, None])

                def grp(t):      # [Na, 32] -> [Na, 4 lane groups, 8]
                    return t.reshape(Na, 2, 4, 4).permute(0, 2, 1, 3).reshape(Na, 4, 8)
                svg, vg, pg = grp(sv), grp(valid_lse), grp(ispos)
                ps = ps + torch.where(pg, svg, torch.zeros(())).sum(-1)
                pc = pc + pg.sum(-1).to(F32)
                tmax = torch.where(vg, svg, torch.full((), -math.inf)).max(-1).values
                upd = tmax > -math.inf
                mn = torch.maximum(run_m, tmax)
                l = run_l if self.wrong == "no_rescale" else run_l * _exp(run_m - mn)
                l = l + torch.where(vg, _exp(svg - mn[..., None]), torch.zeros(())).sum(-1)
                run_m, run_l = torch.where(upd, mn, run_m), torch.where(upd, l, run_l)
            # the two shuffle steps: lanes ^ 16, then ^ 32
            m01, l01 = self._combine(run_m[:, 0], run_l[:, 0], run_m[:, 1], run_l[:, 1])
            m23, l23 = self._combine(run_m[:, 2], run_l[:, 2], run_m[:, 3], run_l[:, 3])
            m, l = self._combine(m01, l01, m23, l23)
            if o0 >= o1 and self.wrong == "empty_split_zero":
                m = torch.zeros(Na)
            parts.append((m, l, (ps[:, 0] + ps[:, 1]) + (ps[:, 2] + ps[:, 3]), pc.sum(1)))
        m, l = torch.full((Na,), -math.inf), torch.zeros(Na)
        ps, pc = torch.zeros(Na), torch.zeros(Na)
        for m2, l2, ps2, pc2 in self._order(parts):
            mn = torch.maximum(m, m2)
            l = torch.where(mn > -math.inf, l * _exp(m - mn) + l2 * _exp(m2 - mn), l)
            m, ps, pc = mn, ps + ps2, pc + pc2
        L = m + _log(l)
        has = pc > 0
        ratio = torch.tensor(tau / tau_base, dtype=F32)
        rows_ = torch.where(has, -ratio * (ps / pc.clamp_min(1) - L), torch.zeros(()))
        invcnt = torch.where(has, 1.0 / pc.clamp_min(1), torch.full((), -1.0))
        loss = rows_.sum() * torch.tensor(scale, dtype=F32)
        return dict(loss=loss.reshape(1), lse=L, invcnt=invcnt, rows=rows_)

    def _pass(self, mode, own, other, n_own, n_other, si, ak, ck, lse, invcnt, wscale, inv_temp):
        """One backward mode -> the list of per-split slabs [n_own, D]."""
        ns, per = bwd_geometry(n_own, n_other)
        D = own[0].shape[1]
        own_idx = torch.arange(n_own)
        if mode == "C":       # other rows are anchors: their constants, padded past the end
            def padded(t, fill):
                return torch.cat([t, torch.full((OTHER_TILE,), fill, dtype=t.dtype)])
            o_self, o_key = padded(si, -1), padded(ak, -(2 ** 40))
            o_lse, o_ic = padded(lse, 0.0), padded(invcnt, -1.0)
        else:
            ckp = self._pad_keys(ck)
        slabs = []
        for s in range(ns):
            o0, o1 = s * per, min((s + 1) * per, n_other)
            acc2 = torch.zeros(n_own, D)
            for ob in self._order(range(o0, o1, OTHER_TILE)):
                rows = torch.arange(ob, ob + OTHER_TILE)
                oh, ol = self._tile(other, ob, o1)
                sc = self._prod((oh, ol), own) * inv_temp
                inb = (rows < o1)[None, :]
                if mode == "A":
                    gate = torch.ones(n_own, 1, dtype=torch.bool) if self.wrong == "no_gate_a" else (invcnt >= 0)[:, None]
                    live = inb & (rows[None, :] != si[:, None]) & gate
                    posv = torch.where(ckp[rows][None, :] == ak[:, None], invcnt[:, None], torch.zeros(()))
                    g = wscale * (_exp(sc - lse[:, None]) - posv)
                else:
                    ic = o_ic[rows][None, :]
                    gate = torch.ones(1, OTHER_TILE, dtype=torch.bool) if self.wrong == "no_gate_c" else ic >= 0
                    not_self = (rows[None, :] != own_idx[:, None]) if self.wrong == "base0_in_bwd_c" \
                        else (o_self[rows][None, :] != own_idx[:, None])
                    live = inb & not_self & gate
                    posv = torch.where(o_key[rows][None, :] == ck.long()[:, None], ic, torch.zeros(()))
                    g = wscale * (_exp(sc - o_lse[rows][None, :]) - posv)
                gh, gl = O.split(torch.where(live, g, torch.zeros(())))
                acc2 = acc2 + gh @ oh
                if self.wrong not in ("g_hi_only", "hi_hi_only"):
                    acc2 = acc2 + gl @ oh
                if self.wrong not in ("hi_hi_only", "drop_lo_hi"):
                    acc2 = acc2 + (gl @ oh if self.wrong == "hi_lo_twice" else gh @ ol)
            slabs.append(acc2)
        return slabs

    def _both(self, A, C, si, ak, ck, lse, invcnt, g, tau, tau_base, scale):
        wscale = torch.tensor(scale * (tau / tau_base) / tau, dtype=F32) * torch.tensor(g, dtype=F32)
        inv_temp = torch.tensor(1.0 / tau, dtype=F32)
        a, c = O.split(A), O.split(C)
        si, ak = si.long(), ak.long()
        lse, invcnt = lse.to(F32), invcnt.to(F32)
        Na, N = A.shape[0], C.shape[0]
        return (self._pass("A", a, c, Na, N, si, ak, ck, lse, invcnt, wscale, inv_temp),
                self._pass("C", c, a, N, Na, si, ak, ck, lse, invcnt, wscale, inv_temp))

    def _sum(self, slabs):
        slabs = self._order(slabs)
        out = slabs[0]
        for s in slabs[1:]:
            out = out + s
        return out

    def bwd(self, A, C, si, ak, ck, lse, invcnt, g, tau, tau_base, scale):
        sa, sc = self._both(A, C, si, ak, ck, lse, invcnt, g, tau, tau_base, scale)
        return self._sum(sa), self._sum(sc)

    def bwd_sum(self, X, si, ak, ck, lse, invcnt, g, tau, tau_base, scale):
        sa, sc = self._both(X, X, si, ak, ck, lse, invcnt, g, tau, tau_base, scale)
        return self._sum(sa + sc)


# ---------------------------------------------------------------- comparison ------------------

def within(stats, name, got, ref, bound, ctx="", strict=True):
    """Assert |got − ref| <= bound elementwise (a zero bound demands equality); record the largest
    error / bound under ``name`` in ``stats`` (0/0 counts as 0, x/0 as inf)."""
    got, ref, bound = got.to(F64).reshape(-1), ref.to(F64).reshape(-1), bound.to(F64).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full((), math.inf, dtype=F64))
    ratio = torch.where(err == 0, torch.zeros((), dtype=F64), err / bound)
    worst = ratio.max().item() if ratio.numel() else 0.0
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), worst)
    if strict and not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{name} {ctx}: error / bound = {worst:.4g} at flat index {i}: got "
                             f"{got[i].item():.9g}, ref {ref[i].item():.9g}, bound {bound[i].item():.4g}")
    return worst


def check_case(impl, name, stats=None, strict=True):
    """Forward, two-output backward and (anchors == contrasts) the merged backward of one case
    against split_model; -> the largest error / bound over all outputs."""
    c = cases()[name]
    M = _model(c)
    ctx = f"({name}: Na={c.Na}, N={c.N}, D={c.D}, tau={c.tau}, g={c.g})"
    st = {}
    f = impl.fwd(*c.args())
    within(st, "lse", f["lse"], M["lse"], M["B_lse"], ctx, strict)
    within(st, "invcnt", f["invcnt"], torch.where(M["has"], 1.0 / M["cnt"].clamp_min(1).to(F64), -torch.ones((), dtype=F64)),
           M["B_invcnt"], ctx, strict)
    within(st, "rows", f["rows"], M["rows"], M["B_rows"], ctx, strict)
    within(st, "loss", f["loss"], M["loss"].reshape(1), M["B_loss"].reshape(1), ctx, strict)
    if strict:
        nop = ~M["has"]
        assert (f["invcnt"][nop] == -1).all() and (f["rows"][nop] == 0).all(), f"no-positive rows {ctx}"
    extra = (f["lse"], f["invcnt"], c.g, c.tau, TAU_BASE, c.scale)
    dA, dC = impl.bwd(c.A, c.C, c.self_idx, c.akey, c.ckey, *extra)
    within(st, "dA", dA, M["dA"], M["B_dA"], ctx, strict)
    within(st, "dC", dC, M["dC"], M["B_dC"], ctx, strict)
    if c.same:
        dX = impl.bwd_sum(c.C, c.self_idx, c.akey, c.ckey, *extra)
        within(st, "dX", dX, M["dA"] + M["dC"], M["B_dX"], ctx, strict)
    if strict and (c.g == 0 or not M["has"].any()):
        for t in (dA, dC) + ((dX,) if c.same else ()):
            assert (t == 0).all(), f"gradient not exactly 0 {ctx}"
    if strict and not M["has"].any():
        assert f["loss"].item() == 0, f"loss not exactly 0 {ctx}"
    if stats is not None:
        for k, v in st.items():
            stats[k] = max(stats.get(k, 0.0), v)
    return max(st.values())


def check_repeat(impl, name, repeats=3):
    """Forward outputs and all three backward forms bit-identical over ``repeats`` calls."""
    c = cases()[name]
    X = c.C if c.same else None

    def once():
        f = impl.fwd(*c.args())
        extra = (f["lse"], f["invcnt"], c.g, c.tau, TAU_BASE, c.scale)
        outs = [f["loss"], f["lse"], f["invcnt"], f["rows"], *impl.bwd(c.A, c.C, c.self_idx, c.akey, c.ckey, *extra)]
        # the merged backward exists only where the anchors are the contrasts
        if X is not None:
            outs.append(impl.bwd_sum(X, c.self_idx, c.akey, c.ckey, *extra))
        return outs
    first = once()
    for _ in range(repeats - 1):
        for a, b in zip(first, once()):
            assert torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"not repeatable ({name})"
    return len(first)


def check_wrapper(dev, stats=None):
    """ops.contrastive.supcon_rows_loss: bf16 inputs, a strided A, ``A is C`` (merged backward)
    against ``A = C * 1.0`` (two outputs) inside the bounds of one oracle, gradient dtypes."""
    from simclr_pytorch_distributed_amd.ops.contrastive import supcon_rows_loss
    c = cases()["edge_64x64_D64"]
    M = _model(c)
    gfac = c.g
    si, ak, ck = (t.to(dev) for t in (c.self_idx, c.akey, c.ckey))
    # merged and two-output backward of the same oracle
    X = c.C.to(dev).requires_grad_(True)
    loss, rows = supcon_rows_loss(X, X, si, ak, ck, c.tau, TAU_BASE, c.scale, return_rows=True)
    (loss * gfac).backward()
    Y = c.C.to(dev).requires_grad_(True)
    (supcon_rows_loss(Y * 1.0, Y, si, ak, ck, c.tau, TAU_BASE, c.scale) * gfac).backward()
    assert X.grad.dtype == F32 and Y.grad.dtype == F32
    within(stats, "loss", loss.detach().cpu().reshape(1), M["loss"].reshape(1), M["B_loss"].reshape(1), "(wrapper)")
    within(stats, "rows", rows.cpu(), M["rows"], M["B_rows"], "(wrapper)")
    within(stats, "dX", X.grad.cpu(), M["dA"] + M["dC"], M["B_dX"], "(wrapper, A is C)")
    # two outputs and one fp32 add by autograd: u·(|dA| + |dC|) more
    two = M["B_dA"] + M["B_dC"] + U24 * (M["dA"].abs() + M["dC"].abs())
    within(stats, "dA+dC", Y.grad.cpu(), M["dA"] + M["dC"], two, "(wrapper, A = C * 1.0)")
    # a strided view as A: every other row of a [2·Na, D] tensor
    c2 = cases()["edge_129x257_D64"]
    M2 = _model(c2)
    si2, ak2, ck2 = (t.to(dev) for t in (c2.self_idx, c2.akey, c2.ckey))
    wide = torch.zeros(2 * c2.Na, c2.D, device=dev)
    wide[::2] = c2.A.to(dev)
    wide.requires_grad_(True)
    Av = wide[::2]
    assert not Av.is_contiguous()
    Cg = c2.C.to(dev).requires_grad_(True)
    (supcon_rows_loss(Av, Cg, si2, ak2, ck2, c2.tau, TAU_BASE, c2.scale) * c2.g).backward()
    within(stats, "dA", wide.grad[::2].cpu(), M2["dA"], M2["B_dA"], "(wrapper, strided A)")
    assert (wide.grad[1::2] == 0).all()
    within(stats, "dC", Cg.grad.cpu(), M2["dC"], M2["B_dC"], "(wrapper, strided A)")
    # bf16 inputs: the oracle sees the same bf16 values; the returned gradients are rounded to
    # bf16 once (unit roundoff 2^-8: 8 significant bits) on top of the fp32 bound
    Ab = c2.A.bfloat16()
    Cb = c2.C.bfloat16()
    cb = Case("bf16", Ab.float(), Cb.float(), c2.self_idx, c2.akey, c2.ckey, c2.tau, g=c2.g)
    Mb = _model(cb)
    Ag, Cg = Ab.to(dev).requires_grad_(True), Cb.to(dev).requires_grad_(True)
    loss = supcon_rows_loss(Ag, Cg, si2, ak2, ck2, cb.tau, TAU_BASE, cb.scale)
    (loss * cb.g).backward()
    assert Ag.grad.dtype == torch.bfloat16 and Cg.grad.dtype == torch.bfloat16 and loss.dtype == F32
    within(stats, "loss", loss.detach().cpu().reshape(1), Mb["loss"].reshape(1), Mb["B_loss"].reshape(1), "(wrapper, bf16)")
    for nm, got, key in (("dA", Ag.grad, "dA"), ("dC", Cg.grad, "dC")):
        within(stats, nm + " (bf16)", got.float().cpu(), Mb[key], Mb["B_" + key] * (1 + 2.0 ** -8) + 2.0 ** -8 * Mb[key].abs(),
               "(wrapper, bf16)")
