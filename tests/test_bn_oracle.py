"""CPU tests of the BatchNorm oracle (tests/bn_oracle.py) and of the bounds, cases and grid
mirrors of tests/bn_checks.py: the oracle equals torch autograd in float64, the fp32 twin stays
inside every bound at every named case, every deliberately wrong twin falls outside, and every
case sits on the path it is named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_checks as K
import bn_oracle as O

F64 = torch.float64
EPS32, MOM32 = float(np.float32(K.EPS)), float(np.float32(K.MOMENTUM))


def _close(a, b, rel=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert (a - b).abs().max().item() <= rel * b.abs().max().clamp_min(1e-300).item(), (a - b).abs().max().item()


# ---------------------------------------------------------------- oracle vs autograd ----------

@pytest.mark.parametrize("res_mode", [0, 1, 2])
def test_oracle_matches_autograd(res_mode):
    g = torch.Generator().manual_seed(res_mode)
    N, H, W, C = 3, 5, 4, 16
    n = N * H * W
    ya = (torch.randn(n, C, generator=g) * 2 + 0.5).bfloat16().to(F64)
    yb = (torch.randn(n, C, generator=g) - 1).bfloat16().to(F64)
    dout = torch.randn(n, C, generator=g).bfloat16().to(F64)
    ga, ba, _ = (t.to(F64) for t in K.channel_vectors(C, g))
    gb, bb, _ = (t.to(F64) for t in K.channel_vectors(C, g))
    rm, rv = torch.randn(C, generator=g).to(F64), (torch.rand(C, generator=g) + 0.5).to(F64)

    def nchw(t):
        return t.reshape(N, H, W, C).permute(0, 3, 1, 2)

    ta, tb = nchw(ya).clone().requires_grad_(True), nchw(yb).clone().requires_grad_(True)
    pa = [t.clone().requires_grad_(True) for t in (ga, ba)]
    pb = [t.clone().requires_grad_(True) for t in (gb, bb)]
    rma, rva, rmb, rvb = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    o = F.batch_norm(ta, rma, rva, pa[0], pa[1], training=True, momentum=MOM32, eps=EPS32)
    if res_mode == 1:
        o = o + F.batch_norm(tb, rmb, rvb, pb[0], pb[1], training=True, momentum=MOM32, eps=EPS32)
    elif res_mode == 2:
        o = o + tb
    o = F.relu(o)
    o.backward(nchw(dout))

    fa = O.finalize(O.stats(ya), n, ga, ba, K.EPS, K.MOMENTUM, rm, rv)
    fb = O.finalize(O.stats(yb), n, gb, bb, K.EPS, K.MOMENTUM, rm, rv)
    z, _ = O.apply(ya, fa["scale"], fa["shift"], yb, fb["scale"], fb["shift"], res_mode, relu=True)
    _close(nchw(z), o.detach())
    _close(fa["running_mean"], rma)
    _close(fa["running_var"], rva)
    two = res_mode == 1
    sums, _, dz = O.bwd_sums(dout, ("act", z), ya, fa["mean"], yb if two else None, fb["mean"] if two else None)
    ca = O.coef(sums, n, ga, fa["mean"], fa["invstd"])
    _close(ca["dgamma"], pa[0].grad)
    _close(ca["dbeta"], pa[1].grad)
    cb = O.coef(sums, n, gb, fb["mean"], fb["invstd"], set_index=1) if two else None
    r = O.bwd_apply(dout, ("act", z), ya, torch.stack([ca["A"], ca["D"], ca["E"]]), yb if two else None,
                    torch.stack([cb["A"], cb["D"], cb["E"]]) if two else None)
    _close(nchw(r["dya"]), ta.grad)
    if two:
        _close(fb["running_mean"], rmb)
        _close(fb["running_var"], rvb)
        _close(cb["dgamma"], pb[0].grad)
        _close(cb["dbeta"], pb[1].grad)
        _close(nchw(r["dyb"]), tb.grad)
    if res_mode == 2:
        _close(nchw(dz), tb.grad)


def test_oracle_eval_mode():
    g = torch.Generator().manual_seed(7)
    C = 24
    gamma, beta, rm = (t.to(F64) for t in K.channel_vectors(C, g))
    rv = (torch.rand(C, generator=g) + 0.1).to(F64)
    y = torch.randn(6, C, generator=g).bfloat16().to(F64)
    sc, sh = O.eval_affine(gamma, beta, rm, rv, K.EPS)
    z, _ = O.apply(y, sc, sh, relu=False)
    ref = F.batch_norm(y.reshape(6, C, 1, 1), rm, rv, gamma, beta, training=False, eps=EPS32)
    _close(z, ref.reshape(6, C))


def test_grad_scale_and_count_one():
    s = torch.tensor([[2.0, -3.0], [0.5, 4.0]], dtype=F64)
    inv, mu = torch.tensor([1.5, 0.75]), torch.tensor([0.25, -2.0])
    c1, c4 = O.coef(s, 8, None, mu, inv, 1.0), O.coef(s, 8, None, mu, inv, 0.25)
    _close(c4["dgamma"], 0.25 * c1["dgamma"])
    _close(c4["dbeta"], 0.25 * c1["dbeta"])
    _close(c4["A"], c1["A"])
    f = O.finalize(torch.tensor([[3.0], [9.0]], dtype=F64), 1, None, None, K.EPS, 1.0, torch.zeros(1), torch.ones(1))
    assert f["running_var"].item() == 0.0 and f["running_mean"].item() == 3.0   # no n / (n − 1) at n = 1


# ---------------------------------------------------------------- bf16 helpers ----------------

def test_bf16_round_is_bit_equal_to_torch():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1 << 16, generator=g) * 10.0 ** (torch.rand(1 << 16, generator=g) * 20 - 10)
    # ties: bf16 values plus exactly half a bf16 ulp (low 16 bits 0x8000), both parities, both signs
    base = (torch.randn(4096, generator=g).bfloat16().float().numpy().view(np.uint32) | np.uint32(0x8000))
    ties = torch.from_numpy(base.view(np.float32).copy())
    near = torch.from_numpy((base + np.uint32(1)).view(np.float32).copy())
    below = torch.from_numpy((base - np.uint32(1)).view(np.float32).copy())
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.3895314e38, 1e-40, -1e-40, float("inf"), float("-inf")])
    for t in (x, ties, near, below, edge):
        got, ref = O.bf16_round(t), t.bfloat16().float()
        assert np.array_equal(got.numpy().view(np.uint32), ref.numpy().view(np.uint32))
        assert np.array_equal(O.bf16_bits(got), O.bf16_bits(t.bfloat16()))
    assert (ties.bfloat16().float() != ties).all()


def test_relu_bits_layout_and_zeros():
    v = torch.tensor([1.0, -1.0, 0.0, -0.0, 1e-30, -1e-30, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 5.0])
    bits = O.relu_bits(v.bfloat16())
    assert bits.dtype == np.uint8 and bits.tolist() == [0b11010001, 0b10000000]
    assert O.unpack_bits(bits, 16).tolist() == (v > 0).tolist()


# ---------------------------------------------------------------- twin inside every bound -----

@pytest.mark.parametrize("C,rows", K.EW_CASES + K.EW_KNOB_CASES)
def test_twin_within_bounds_elementwise(C, rows):
    twin = K.TwinImpl()
    K.check_apply(twin, C, rows)
    K.check_bwd_apply(twin, C, rows)


@pytest.mark.parametrize("C,rows", K.REDUCE_CASES)
def test_twin_within_bounds_reduce(C, rows):
    K.check_bwd_reduce(K.TwinImpl(), C, rows, repeats=1)


@pytest.mark.parametrize("g", K.REDUCE3_G)
def test_twin_within_bounds_reduce_three_sets(g):
    K.check_bwd_reduce3(K.TwinImpl(), g, repeats=1)


@pytest.mark.parametrize("C,rows", K.EW_CASES + K.EW_KNOB_CASES + K.REDUCE_CASES + K.REDUCE3_CASES)
def test_recomputed_mask_is_decided_beyond_fp32_rounding(C, rows):
    """No allowance is made for a recomputed mask that fp32 and fp64 decide differently: every
    generated ya·msc + msh is exactly 0 or beyond the reach of a fp32 rounding."""
    d = K.inputs(C, rows)
    assert K.mask_margin_ok(d)
    v = d["ya"].double() * d["msc"].double() + d["msh"].double()
    assert (v == 0).any() or rows * C < 200                    # the exact-zero edge occurs


def test_forward_negative_zero_is_reached():
    """With ReLU off, bn_apply's output holds −0 (y·sc = −0 on a shift of −0), +0 and exact-zero
    values whose mask bit must be clear."""
    for C, rows in [(24, 100), (40, 77), (136, 31)]:
        d = K.inputs(C, rows)
        out = O.twin_apply(d["y"], d["sc"], d["sh"], res_mode=0, relu=False)
        bits = O.bf16_bits(out)
        assert (bits == 0x8000).any() and (bits == 0).any(), (C, rows)
        _, T = O.apply(d["y"], d["sc"], d["sh"], relu=False)
        assert (T == 0).sum() >= (bits == 0x8000).sum() > 0


@pytest.mark.parametrize("C", K.STATS_C)
def test_twin_within_bounds_stats(C):
    for rows in K.stats_rows_for(C):
        K.check_stats(K.TwinImpl(), rows, C, repeats=1)


def test_twin_within_bounds_finalize_edges_and_eval():
    twin = K.TwinImpl()
    K.check_finalize_edges(twin)
    for C in K.EVAL_CASES:
        assert K.eval_affine_error(twin, C) <= K.EVAL_AFFINE_CEILING
        K.check_eval_chain(twin, C)


def test_stat_slab_needs_fp64():
    """The slab columns mix magnitudes so that a float32 reduction misses the bound."""
    slab = K.stat_slab(257, 64)
    ref = slab.to(F64).sum(0)
    err = (slab.sum(0).to(F64) - ref).abs()
    assert (err > 257 * K.U52 * slab.to(F64).abs().sum(0)).any()


# ---------------------------------------------------------------- sensitivity -----------------
# (defect, check, arguments, message): the wrong twin must fall outside the bound it is meant for
# (the start of the assertion's message) at these inputs

SENSITIVITY = [
    ("rotate_in_group", K.check_apply, dict(C=8, rows=5), r"^bn_apply \("),
    ("rotate_in_group", K.check_bwd_apply, dict(C=8, rows=5, kinds=["none"]), r"^bn_bwd_apply \("),
    ("rotate_in_group", K.check_bwd_reduce, dict(C=8, rows=5, kinds=["affine"], repeats=1), r"^bn_bwd_reduce \("),
    ("next_group", K.check_apply, dict(C=16, rows=33), r"^bn_apply \("),
    ("next_group", K.check_apply, dict(C=24, rows=100), r"^bn_apply \("),
    ("next_group", K.check_bwd_apply, dict(C=24, rows=100, kinds=["act"]), r"^bn_bwd_apply \("),
    ("next_group", K.check_bwd_reduce, dict(C=16, rows=33, kinds=["none"], repeats=1), r"^bn_bwd_reduce \("),
    ("mode1_as_mode2", K.check_apply, dict(C=40, rows=77, modes=(1,)), r"^bn_apply \("),
    ("mean_b_for_a", K.check_bwd_reduce, dict(C=16, rows=33, kinds=["bits"], sets=(True,), repeats=1), r"^bn_bwd_reduce \("),
    ("biased_var", K.check_stats, dict(rows=33, C=40, repeats=1), r"^bn_finalize running_var"),
    ("biased_var", K.check_finalize_edges, dict(), r"^bn_finalize running_var"),
    ("count_minus_one", K.check_stats, dict(rows=33, C=40, repeats=1), r"^bn_finalize mean"),
    ("mask_ge", K.check_bwd_apply, dict(C=8, rows=5, kinds=["act"]), r"^bn_bwd_apply dz not bit-equal"),
    ("mask_ge", K.check_bwd_apply, dict(C=16, rows=33, kinds=["affine"]), r"^bn_bwd_apply dz not bit-equal"),
    ("mask_ge", K.check_bwd_reduce, dict(C=16, rows=33, kinds=["act"], repeats=1), r"^bn_bwd_reduce \("),
    ("dbeta_unscaled", K.check_bwd_reduce, dict(C=8, rows=5, kinds=["act"], repeats=1), r"^bn_bwd_coef dbeta"),
    ("overwrite_sinks", K.check_bwd_reduce, dict(C=8, rows=5, kinds=["none"], repeats=1), r"^bn_bwd_reduce_coef dgamma"),
    ("drop_tail", K.check_apply, dict(C=16, rows=33), r"^bn_apply \("),
    ("drop_tail", K.check_bwd_apply, dict(C=16, rows=33, kinds=["none"]), r"^bn_bwd_apply dz not bit-equal"),
    ("drop_tail", K.check_bwd_reduce, dict(C=128, rows=4097, kinds=["none"], sets=(False,), repeats=1), r"^bn_bwd_reduce \("),
    ("drop_tail", K.check_stats, dict(rows=5, C=8, repeats=1), r"^bn_stats_reduce"),
]


@pytest.mark.parametrize("defect,check,kw,message", SENSITIVITY, ids=[f"{d}-{c.__name__}-{i}" for i, (d, c, _, _) in enumerate(SENSITIVITY)])
def test_wrong_twin_is_caught(defect, check, kw, message):
    check(K.TwinImpl(), **kw)                       # the correct twin passes at these inputs
    with pytest.raises(AssertionError, match=message):
        check(K.TwinImpl({defect}), **kw)


def test_every_defect_is_listed():
    assert {d for d, _, _, _ in SENSITIVITY} == {
        "rotate_in_group", "next_group", "mode1_as_mode2", "mean_b_for_a", "biased_var", "count_minus_one",
        "mask_ge", "dbeta_unscaled", "overwrite_sinks", "drop_tail"}


# ---------------------------------------------------------------- cases sit on their paths ----

@pytest.fixture
def default_knobs(monkeypatch):
    for k in K.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)


def test_elementwise_cases_hit_their_paths(default_knobs):
    # (C, rows) -> (fast branch, fewest, most grid-stride iterations), forward and backward alike
    expect = {(8, 5): (True, 0, 1), (16, 33): (True, 0, 1), (24, 100): (False, 0, 1), (24, 256): (True, 1, 1),
              (40, 77): (False, 0, 1), (136, 31): (False, 0, 1), (2048, 3): (True, 1, 1), (4096, 2): (True, 1, 1),
              (1024, 5115): (True, 1, 2), (24, 250000): (False, 1, 2), (24, 3000): (True, 0, 1), (64, 1000): (True, 0, 1)}
    assert set(expect) == set(K.EW_CASES + K.EW_KNOB_CASES)
    for (C, rows), path in expect.items():
        assert K.ew_path(C, rows) == path and K.ew_path(C, rows, bwd=True) == path, (C, rows)
    assert K.ew_grid(24 * 100 // 8) == 2 and 512 % 3 != 0          # g = 2
    assert K.ew_grid(24 * 256 // 8) == 3                           # g = 3 on the fast branch
    assert 1024 * 5115 // 8 > 2048 * 256 and K.ew_grid(1024 * 5115 // 8) == 2048
    assert [C // 8 for C, _ in K.EW_CASES[:8]] == [1, 2, 3, 3, 5, 17, 256, 512]
    assert 5 * 8 // 8 < 256 and (16 * 33 // 8) % 256 != 0          # n8 < 256, partial block
    assert max(C * rows for C, rows in K.EW_CASES) <= 6_000_000


def test_elementwise_cases_under_the_knobs(monkeypatch):
    for k, v in K.KNOB_ENV.items():
        monkeypatch.setenv(k, v)
    assert K.ew_cap() == 8 and K.ew_cap(True) == 16
    assert K.ew_path(24, 3000) == (False, 4, 5) and K.ew_path(24, 3000, bwd=True) == (False, 2, 3)
    assert K.ew_path(64, 1000) == (True, 3, 4) and K.ew_path(64, 1000, bwd=True) == (True, 1, 2)
    assert K.col_reduce_gy(9) == 12 and K.col_reduce_per(9) == 1   # blocks 9..11 have no rows
    monkeypatch.setenv("SDX_EW_BLOCKS", "7")                       # below 8: ignored
    monkeypatch.delenv("SDX_EW_BLOCKS_BWD")
    assert K.ew_cap() == 2048 and K.ew_cap(True) == 2048
    monkeypatch.setenv("SDX_EW_BLOCKS", "21")                      # rounded down to a multiple of 8
    assert K.ew_cap() == 16 and K.ew_cap(True) == 16


def test_reduce_cases_hit_their_paths(default_knobs):
    # (C, rows) -> (blocks g, chunks per thread n_t, threads sharing a channel group in a block)
    expect = {(8, 5): (1, 1, 256), (16, 33): (1, 1, 128), (64, 1): (1, 1, 32), (512, 9): (1, 3, 4),
              (1024, 7): (1, 4, 2), (2048, 1): (1, 1, 1), (2048, 3): (1, 3, 1), (128, 4097): (17, 16, 16)}
    assert set(expect) == set(K.REDUCE_CASES)
    for (C, rows), (g, n_t, share) in expect.items():
        assert (K.bn_bwd_reduce_blocks(C * rows), K.reduce_n_t(rows, C), 256 // (C // 8)) == (g, n_t, share), (C, rows)
    assert (128 * 4097 // 8) % (17 * 256) != 0                     # ragged last stride
    assert K.col_reduce_gy(17) == 2                                # the partial slab's own reduction


def test_three_set_reduce_cases_hit_their_paths(default_knobs):
    """The partial slab of bn_bwd_reduce has g rows: g sits on the row table of the column
    reduction (as far as 6.4 M elements reach), with its gy and rows per block."""
    # g -> (gy, rows per block)
    expect = {3: (1, 3), 4: (1, 4), 5: (1, 5), 8: (1, 8), 9: (2, 5), 31: (3, 11), 32: (3, 11), 33: (3, 11),
              36: (3, 12), 37: (3, 13), 127: (6, 22), 128: (6, 22), 197: (7, 29)}
    assert set(expect) == set(K.REDUCE3_G)
    for g, (gy, per) in expect.items():
        C, rows = K.reduce3_case(g)
        assert C in (8, 64) and K.bn_bwd_reduce_blocks(C * rows) == g, g
        assert (K.col_reduce_gy(g), K.col_reduce_per(g)) == (gy, per), g
        assert 11 <= K.reduce_n_t(rows, C) <= 16 and (rows * C // 8) % (256 * g) != 0
        assert C * rows <= 6_500_000
    # more than 28 rows per block (the unrolled trip) first at g = 197; its tail (33 rows per
    # block) first at g = 257 = 8.4 M elements; gy = 64 needs g = 16129 > the cap of 1024
    assert min(g for g in range(1, 1025) if K.col_reduce_per(g) > 28) == 197
    assert min(g for g in range(1, 1025) if K.col_reduce_per(g) >= 33) == 257 and 257 * 4096 * 8 > 8_000_000
    assert K.bn_bwd_reduce_blocks(2 ** 40) == 1024 and K.col_reduce_gy(1024) == 16


def test_stats_rows_hit_their_paths(default_knobs):
    gy = {r: K.col_reduce_gy(r) for r in K.STATS_ROWS + K.STATS_ROWS_MAXY}
    per = {r: K.col_reduce_per(r) for r in gy}
    assert gy[8] == 1 and gy[9] == 2                               # 9 is where gy becomes 2
    assert gy[16128] == 63 and gy[16129] == 64                     # the MAXY limit of the combine
    assert K.col_reduce_gy(10 ** 6) == 64
    assert per[1] == 1 and per[3] == 3 and per[4] == 4 and per[5] == 5      # rows per block around 4
    assert (gy[36], per[36], gy[37], per[37]) == (3, 12, 3, 13)
    # the 32-row unrolled trip (8 rows x 4 thread rows): thread row ty takes it iff per > 28 + ty
    assert (per[196], per[197], per[224], per[257]) == (28, 29, 32, 33)
    assert per[16128] == 256 and per[16129] == 253
    assert 16129 - 63 * per[16129] == 190                          # a ragged last block
    for C in K.STATS_C:
        assert all(r <= 33 for r in K.stats_rows_for(C)) or C != 4096
    assert [(C + 63) // 64 * 64 == C for C in K.STATS_C] == [False, False, True, False, False, True]
