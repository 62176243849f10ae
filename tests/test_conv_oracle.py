"""The conv oracle and its checks, on the CPU: the fp64 oracle of tests/conv_oracle.py agrees with
fp64 torch autograd, every case of tests/conv_checks.py meets the < 2^24 exactness guard in both
regimes, the fp32 twin passes every comparison, each deliberate defect fails one — and the
truncating store passes the norm the older conv tests use, which is why these tests exist —
and every case sits on the dispatch path it is named for (host-only ``conv_plan``)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_checks as K
import conv_oracle as O

F32, F64 = torch.float32, torch.float64
TWIN = K.TwinImpl()
TAP_SHAPES = [(n, h, h, c, k, 3, 1, 1) for n, h, c, k in K.TAP_CASES]
ALL_SHAPES = list(K.FWD_CASES.values()) + TAP_SHAPES
WGRAD_SHAPES = [s for s, _ in K.WGRAD_3X3] + [r[0] for r in K.WGRAD_1X1] + [(33, 8, 8, 64, 64, 1, 1, 0),
                                                                            (4, 8, 8, 8, 24, 1, 1, 0)]


# ---------------------------------------------------------------- rne_bf16 --------------------

def test_rne_bf16_ties_and_neighbours():
    """257 = 1.00000001b·2^8 lies halfway between 256 and 258: to even, 256; 259 halfway between
    258 and 260: to even, 260. One fp32 ulp beside a tie goes to the near side."""
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, 260.0, 261.0, -257.0, -259.0, 0.0, 1.0, -4.0, 23555.0, 0.5], dtype=F64)
    want = torch.tensor([256.0, 256.0, 258.0, 260.0, 260.0, 260.0, -256.0, -260.0, 0.0, 1.0, -4.0, 23552.0, 0.5], dtype=F64)
    assert torch.equal(O.rne_bf16(t), want)
    ulp = 2.0 ** -15                                   # fp32 ulp in [256, 512)
    beside = torch.tensor([257.0 - ulp, 257.0 + ulp, 259.0 - ulp, 259.0 + ulp], dtype=F64)
    assert torch.equal(O.rne_bf16(beside), torch.tensor([256.0, 258.0, 258.0, 260.0], dtype=F64))
    assert torch.equal(O.trunc_bf16(torch.tensor([257.0, 259.0, -259.0, 259.0 + ulp], dtype=F64)),
                       torch.tensor([256.0, 258.0, -258.0, 258.0], dtype=F64))
    # every fp32 pattern of a stretch around a binade edge, against torch's own cast
    u = np.arange(0x437F0000, 0x43810000, 37, dtype=np.uint32)
    f = torch.from_numpy(u.view(np.float32).copy())
    assert torch.equal(O.rne_bf16(f.to(F64)), f.bfloat16().to(F64))
    with pytest.raises(AssertionError):
        O.rne_bf16(torch.tensor([1.0 + 2.0 ** -30], dtype=F64))


# ---------------------------------------------------------------- oracle vs torch autograd ----

@pytest.mark.parametrize("shape", ALL_SHAPES + WGRAD_SHAPES[:6])
def test_oracle_matches_fp64_autograd(shape):
    N, H, W, C, Kc, R, st, pad = shape
    d = K.inputs(shape, "wide")
    x = d["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = d["w"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(x, w, stride=st, padding=pad)
    dx, dw = torch.autograd.grad(y, (x, w), d["dy"].permute(0, 3, 1, 2))
    assert torch.equal(O.fwd_acc(d["x"], d["w"], st, pad), y.detach().permute(0, 2, 3, 1))
    assert torch.equal(O.dgrad_acc(d["dy"], d["wt"], H, W, st, pad), dx.permute(0, 2, 3, 1))
    assert torch.equal(O.wgrad(d["dy"], d["x"], R, R, st, pad), dw.permute(0, 2, 3, 1))


# ---------------------------------------------------------------- twin passes, guard holds ----

def _all_checks(impl, shapes=None, regimes=K.REGIMES):
    """Every comparison at a reduced cfg list (the twin has no tiles); returns nothing, raises."""
    for regime in regimes:
        for shape in shapes or ALL_SHAPES:
            K.check_fwd(impl, shape, regime)
            K.check_dgrad(impl, shape, regime)
        for shape in K.EPI_SHAPES:
            K.check_fwd(impl, shape, regime, prologue=True)
            K.check_wgrad(impl, shape, regime, -2, 0, prologue=True)
            for a in K.ADDENDS[1:]:
                K.check_dgrad(impl, shape, regime, addend=a)
        for shape in K.BIAS_SHAPES:
            for relu in (True, False):
                K.check_fwd_bias(impl, shape, regime, relu)
        for case in K.CAT_CASES:
            K.check_dgrad_cat(impl, case, regime)
        for shape in K.BNSTAT_SHAPES:
            for mask in K.MASKS:
                for sets in (1, 2):
                    K.check_dgrad_bnstat(impl, shape, regime, sets=sets, mask=mask)
            K.check_dgrad_bnstat(impl, shape, regime, mask="bits", addend="masked", extra_rows=3)
            K.check_dgrad_bnstat(impl, shape, regime, mask="bits", no_ya=True)
            if shape[6] == 1:
                K.check_dgrad_bnstat(impl, shape, regime, sets=2, mask="bits", store_masked=1)
        for shape, cfg in K.WGRAD_GENERIC:
            for splits, sink in K.wgrad_variants(impl, shape, cfg, shape[0] * K.out_hw(shape)[0] * K.out_hw(shape)[1]):
                K.check_wgrad(impl, shape, regime, cfg, splits, sink)
            K.check_wgrad(impl, shape, regime, cfg, 0, "cl", accumulate=False)


def test_twin_passes_every_comparison_and_guard_holds():
    _all_checks(TWIN)
    for regime in K.REGIMES:
        for shape in TAP_SHAPES:
            K.check_dgrad_bnstat(TWIN, shape, regime, mask="bits")
        for shape in WGRAD_SHAPES:
            K.check_wgrad(TWIN, shape, regime, -1, 3, "krsc")
    worst = K.GUARD.worst
    print({k: f"{v:.6g}" for k, v in worst.items()})
    assert worst and all(v < K.LIMIT for v in worst.values())


def test_wide_regime_really_rounds():
    """A fifth of |y| and more is above 256 in the wide regime at Kdim >= 1152: the bf16 store
    rounds, ties included."""
    for shape in (K.FWD_CASES["ragged M, 18 K-tiles"], (3, 4, 4, 512, 512, 3, 1, 1)):
        acc = K.ref_fwd(shape, "wide")["acc"]
        assert (acc.abs() > 256).double().mean() > 0.05
        assert (O.rne_bf16(acc) != acc).any() and (O.rne_bf16(acc) != O.trunc_bf16(acc)).any()
        odd = acc.abs() > 256
        assert ((acc[odd] % 4).abs() == 2).any() or ((acc[odd] % 2) == 1).any()      # ties present


# ---------------------------------------------------------------- defects are caught ----------

def _mk(N, H, W, C, Kc, R, seed=0):
    """The Gaussian inputs of tests/test_gpu_conv.py (NCHW)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).bfloat16()
    w = (torch.randn(Kc, C, R, R, generator=g) / (C * R * R) ** 0.5).bfloat16()
    return x, w


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()


OLD_SHAPES = [(2, 4, 4, 512, 512, 3, 1, 1), (8, 16, 16, 128, 256, 3, 1, 1), (4, 8, 8, 64, 64, 1, 1, 0)]


def old_norm(defect):
    """The older tests' norm max|got − ref| / max|ref| of the defective twin on their Gaussian
    inputs, worst over OLD_SHAPES -> (value, limit): forward y for the store / reduction defects
    (limit 1e-2), dx with an addend for the addend defect (1e-2), dW (5e-3) for the others."""
    impl = K.TwinImpl([defect])
    worst = 0.0
    for shape in OLD_SHAPES:
        N, H, W, C, Kc, R, st, pad = shape
        x, w = _mk(N, H, W, C, Kc, R)
        xh, wh = x.permute(0, 2, 3, 1).to(F64), w.permute(0, 2, 3, 1).to(F64)
        ref = F.conv2d(x.float(), w.float(), stride=st, padding=pad)
        g = torch.Generator().manual_seed(1)
        dy = torch.randn(ref.shape, generator=g).bfloat16()
        dyh = dy.permute(0, 2, 3, 1).to(F64)
        if defect in ("trunc_store", "stats_from_stored", "tail_k_channel", "pad_tap_neighbour"):
            acc = impl._acc(xh, wh, st, pad, None, None).to(F32)      # not exact here: fp32 as the kernel
            got = impl.round(acc.to(F64))
            worst, limit = max(worst, _rel(got.permute(0, 3, 1, 2), ref)), 1e-2
        elif defect == "addend_pre":
            add = torch.randn(N, H, W, C, generator=g).bfloat16().to(F64)
            wt = wh.permute(3, 1, 2, 0).contiguous()
            acc = impl._dacc(dyh, wt, H, W, st, pad).to(F32).to(F64)
            got = impl._dfin(acc, add, None, 0)
            exp = acc + add
            worst, limit = max(worst, _rel(got, exp)), 1e-2
        else:
            wf = w.float().requires_grad_(True)
            (dw_ref,) = torch.autograd.grad(F.conv2d(x.float(), wf, stride=st, padding=pad), wf, dy.float())
            sink = torch.full((Kc, R, R, C), 0.25, dtype=F64)     # as the older tests' sinks
            got = impl.wgrad(dyh, xh, R, st, pad, 3, -1, sink) - 0.25
            worst, limit = max(worst, _rel(got.permute(0, 3, 1, 2), dw_ref)), 5e-3
    return worst, limit


def _caught(defect):
    impl = K.TwinImpl([defect])
    s1, s2 = K.EPI_SHAPES
    stem = K.FWD_CASES["7x7 stem"]
    runs = {
        "trunc_store": lambda: K.check_fwd(impl, s1, "wide"),
        "stats_from_stored": lambda: K.check_fwd(impl, s1, "wide"),
        "addend_pre": lambda: K.check_dgrad(impl, s1, "wide", addend="full"),
        "split_drop_pixel": lambda: K.check_wgrad(impl, s1, "unit", -2, 2),
        "tail_k_channel": lambda: K.check_fwd(impl, stem, "unit"),
        "pad_tap_neighbour": lambda: K.check_fwd(impl, s1, "unit"),
        "dup_split": lambda: K.check_wgrad(impl, s1, "unit", -2, 2),
        "sink_overwrite": lambda: K.check_wgrad(impl, s1, "unit", -2, 2, "krsc"),
    }
    try:
        runs[defect]()
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_each_defect_fails_a_comparison(defect):
    msg = _caught(defect)
    assert msg is not None, f"{defect}: not caught"
    value, limit = old_norm(defect)
    print(f"{defect}: caught ({msg[:160]}); the old norm gives {value:.4g} against its limit {limit:g}: "
          f"{'passes' if value < limit else 'fails'}")
    if defect == "trunc_store":
        # the reason these tests exist: truncation instead of round-to-nearest-even of every stored
        # output passes the norm of tests/test_gpu_conv.py
        assert value < limit


# ---------------------------------------------------------------- every case on its path ------

@pytest.fixture(scope="module")
def m():
    from simclr_pytorch_distributed_amd.ops import _ext
    mod = _ext.ext()
    if mod is None or not hasattr(mod, "conv_plan"):
        pytest.skip("native extension not built")
    return mod


def test_fwd_dgrad_cases_on_their_paths(m):
    P = lambda kind, name, **kw: K.plan(m, kind, K.FWD_CASES[name], **kw)   # noqa: E731
    p = P("fwd", "ragged M, 18 K-tiles")
    assert (2 * 9 * 7) % K.TILE_M[p["cfg"]] != 0 and 9 * 128 // 64 == 18 and p["depth"] == [3] and p["one"] == [0]
    p = P("fwd", "3 K-tiles, ragged N")
    assert 192 // 64 == 3 and p["one"] == [1] and all(320 % K.TILE_N[c] for c in (0, 2, 4, 5, 6))
    p = P("dgrad", "merged classes")
    assert p["merged"] and len(p["merged_mt"]) == 4 and len(p["depth"]) == 1
    p = P("dgrad", "strided 1x1")
    assert not p["merged"] and len(p["depth"]) == 4 and p["class_mt"].count(0) == 0
    for name, classes in (("odd stride 2", 4), ("odd stride 3", 9)):
        p = P("dgrad", name)
        assert sum(1 for t in p["class_mt"] if t) == classes and p["merged"] == (classes == 4)
    p = P("fwd", "Kdim 72")
    assert 3 * 3 * 8 == 72 and p["tap"][0] == 0 and p["depth"] == [3]
    assert P("dgrad", "Kdim 72")["cfg"] == 11               # its dgrad reduces over K = 64: a tap tile
    p = P("fwd", "7x7 stem")
    assert 7 * 7 * 8 == 392 and 392 % 64 != 0 and p["depth"] == [3] and p["one"] == [0]
    assert K.plan(m, "wgrad", K.FWD_CASES["7x7 stem"])["family"] == "generic"
    p = P("fwd", "auto cfg 6 on DEPTH 6")
    assert p["cfg"] == 6 and p["depth"] == [6]
    for cfg in (5, 6):      # pinned, the 8-wave tiles run DEPTH 6 at more than two K-tiles
        assert P("fwd", "ragged M, 18 K-tiles", cfg=cfg)["depth"] == [6]
        assert P("dgrad", "ragged M, 18 K-tiles", cfg=cfg)["depth"] == [6]
    for mode, kind, lims in ((0, "fwd", (64, 4096)), (1, "dgrad", (32, 4096))):
        got = []
        for lim in lims:
            prev = m.igemm_one_k_set(mode, lim)
            try:
                p = P(kind, "single-stage DEPTH 3")
                got.append((p["depth"], p["one"]))
            finally:
                m.igemm_one_k_set(mode, prev)
        assert got == [([3], [0]), ([3], [1])], (kind, got)
    for cfg in K.PINNED_CFGS[1:]:
        for shape in K.FWD_CASES.values():
            assert K.plan(m, "fwd", shape, cfg)["ok"] and K.plan(m, "dgrad", shape, cfg)["ok"]


def test_tap_cases_on_their_tiles(m):
    for case, shape in zip(K.TAP_CASES, TAP_SHAPES):
        f, d = K.plan(m, "fwd", shape), K.plan(m, "dgrad", shape)
        assert (f["cfg"], d["cfg"]) == K.TAP_CFG[case], case
        assert K.plan(m, "dgrad", shape, bnstat=True)["cfg"] == d["cfg"]
    assert K.plan(m, "fwd", TAP_SHAPES[6])["tap"][0] == 64          # padded rows of 64 virtual pixels
    assert all(K.plan(m, "fwd", s)["tap"][0] == 0 for s in TAP_SHAPES[:6])
    p = K.plan(m, "fwd", TAP_SHAPES[3])
    assert p["tap"][2] == 4 and 5 % 4 == 1                          # 4 images per tile: the last holds one


def _smallest_n(m, shape, cfg):
    for n in range(1, shape[0] + 1):
        try:
            K.plan(m, "wgrad", (n,) + tuple(shape[1:]), cfg)
            return n
        except RuntimeError:
            pass
    return None


def test_wgrad_cases_on_their_kernels(m):
    for shape, cfg in K.WGRAD_GENERIC:
        p = K.plan(m, "wgrad", shape, cfg)
        assert p["family"] == "generic" and (cfg < 0 or p["cfg"] == cfg)
    slots = {}
    for shape, variant in K.WGRAD_3X3:
        p = K.plan(m, "wgrad", shape, 9)
        assert (p["family"], p["variant"]) == ("3x3", variant), shape
        assert _smallest_n(m, shape, 9) == shape[0], shape
        assert K.plan(m, "wgrad", shape, -1)["family"] == "3x3"
        slots.setdefault(variant, []).append(K.out_hw(shape)[1])
    assert slots == {"plain": [32, 16, 8, 4], "pad": [7, 12, 14, 28, 56], "s2": [32, 16, 8, 4], "s2pad": [7, 12, 14, 28]}
    for shape, variant, bn, setter in K.WGRAD_1X1:
        with K.knob(m, *(setter or (None, None))):
            p = K.plan(m, "wgrad", shape, 10)
            assert (p["family"], p["variant"], p["bn"]) == ("1x1", variant, bn), shape
            assert p["pairs"] == (1 if setter and "pairs" in setter[0] else 0)
            assert _smallest_n(m, shape, 10) == shape[0], shape
    for (shape, cfg) in K.DEFER_JOBS:
        p = K.plan(m, "wgrad", shape, cfg, splits=2, accumulate=True)
        assert p["splits"] == 2 and not p["direct"]
    assert len({K.plan(m, "wgrad", s, c, splits=2)["family"] for s, c in K.DEFER_JOBS}) == 3


def test_splitk_counts_reachable(m):
    for n in K.SPLITK_COUNTS:
        for Kc, C in ((64, 64), (24, 8)):
            p = K.plan(m, "wgrad", (n, 8, 8, C, Kc, 1, 1, 0), -1, splits=n)
            assert p["family"] == "generic" and p["splits"] == n and p["direct"] == (n == 1)
    assert (24 * 8 // 4) % 64 != 0
    p = K.plan(m, "wgrad", (33, 8, 8, 64, 64, 1, 1, 0), -1, splits=2)
    assert p["splits"] == 2 and p["per"] == 17 * 64 and 33 * 64 % p["per"] != 0      # a short last split
