"""CPU side of the max-pool, weight-prep and probe-step oracle tests: the fp64 oracles of
tests/aux_oracle.py against float64 torch, the exactness guards of every case, the fp32 twins of
tests/aux_checks.py held to the very comparisons the kernels face in
tests/test_gpu_aux_oracle.py, and every deliberate defect failing its named case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_checks as K
import aux_oracle as O
from conv_oracle import rne_bf16

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def twin():
    return K.TwinImpl()


# ------------------------------------------------------------------ the oracle against torch --

@pytest.mark.parametrize("name", list(K.POOL_CASES))
def test_pool_oracle_matches_torch(name):
    """Values, first-max positions (ties, ±0, ±inf and the all-(-inf) edge windows included) and
    the autograd gradient of float64 F.max_pool2d."""
    d = K.pool_inputs(name)
    k, s, p = d["k"], d["s"], d["p"]
    xt = d["x"].to(F64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y, at = F.max_pool2d(xt, k, s, p, return_indices=True)
    y_ref, pos = O.maxpool_fwd(d["x"], k, s, p)
    assert torch.equal(y.detach().permute(0, 2, 3, 1), y_ref)
    assert torch.equal(K.torch_pos(at, d["W"], k, s, p).permute(0, 2, 3, 1), pos)
    for dy in (d["dy_exact"], d["dy_wide"]):
        xt.grad = None
        y.backward(dy.to(F64).permute(0, 3, 1, 2), retain_graph=True)
        dx, mag, cnt = O.maxpool_bwd(pos, dy, d["H"], d["W"], k, s, p)
        assert torch.allclose(xt.grad.permute(0, 2, 3, 1), dx, rtol=0, atol=1e-12)
    assert int(cnt.max()) <= (-(-k // s)) ** 2
    K.guard_pool(d)


def test_pool_cases_cover_what_they_are_named_for():
    names = list(K.POOL_CASES)
    for k, s, p in K.GEOMS:
        assert any(n.startswith(f"k{k}s{s}p{p} ") for n in names)
    for C in (8, 24, 64):
        for N in (1, 3):
            assert any(f"N{N} C{C}" in n for n in names)
    d = K.pool_inputs(K.UNCOVERED_CASE)
    _, pos = O.maxpool_fwd(d["x"], 3, 3, 0)
    _, _, cnt = O.maxpool_bwd(pos, d["dy_exact"], 8, 8, 3, 3, 0)
    assert (cnt[:, 6:] == 0).all() and (cnt[:, :, 6:] == 0).all()      # rows and columns no window covers
    d = K.pool_inputs(K.NEG_INF_CASE)
    y, pos = O.maxpool_fwd(d["x"], 3, 2, 1)
    assert (y[0, 0, 0:2] == float("-inf")).all() and (pos[0, 0, 0] == 4).all() and (pos[0, 0, 1] == 3).all()
    d = K.pool_inputs("k5s2p2 2x5 N3 C8")                               # H < k
    assert d["H"] < d["k"]
    x = torch.cat([K.pool_inputs(n)["x"].reshape(-1) for n in names])
    assert (x == 0).any() and torch.signbit(x[x == 0]).any() and (~torch.signbit(x[x == 0])).any()
    assert (x == float("inf")).any() and (x == float("-inf")).any() and not torch.isnan(x).any()


def test_wprep_oracle_matches_torch():
    """The layouts against permute + cast, and ConvWeightCache's own per-conv torch conversion."""
    t = K.wprep_table("all, listed order")
    wc = t["wc"]
    assert not wc.native
    wc.buf.view(torch.int16).fill_(K.SENT_BITS)
    wc.refresh()
    for cv, w in zip(t["convs"], t["weights"]):
        e = wc.entries[id(cv)]
        fwd, tr = O.wprep_layouts(w, e["Cp"])
        w4 = w.reshape(e["K"], e["C"], e["R"], e["S"])
        krsc = w4.permute(0, 2, 3, 1).to(torch.bfloat16)
        assert torch.equal(fwd[..., :e["C"]], krsc.to(F64)) and not fwd[..., e["C"]:].any()
        assert torch.equal(tr, krsc.permute(3, 1, 2, 0).to(F64))
        assert np.array_equal(K._bits(wc.fwd(cv).to(F64)), K._bits(fwd))
        if e["off_t"] >= 0:
            assert np.array_equal(K._bits(wc.dgrad(cv).to(F64)), K._bits(tr))
    assert torch.equal(rne_bf16(torch.tensor([1.00390625, 1.01171875], dtype=F64)),
                       torch.tensor([1.0, 1.015625], dtype=F64))       # ties to even, both parities


def test_wprep_tables_cover_the_branches():
    seen = set()
    for name in K.WPREP_TABLES:
        t = K.wprep_table(name)
        rows = t["wc"].seg_rows
        assert [r[6] for r in rows] == sorted(r[6] for r in rows) and rows[0][6] == 0
        for r in rows:
            Kk, C, Cp = r[3] & 0xFFFFFFFF, r[4] & 0xFFFFFFFF, r[4] >> 32
            vec = C % 4 == 0 and Cp == C and Kk % 4 == 0
            seen.add(("vec" if vec else "scalar", "t" if r[2] >= 0 else "no t",
                      "ragged" if Kk % 64 or Cp % 64 else "full"))
    assert {("vec", "t", "ragged"), ("scalar", "t", "ragged"), ("scalar", "no t", "ragged")} <= seen
    assert K.wprep_table("all, a padded stem last")["wc"].seg_rows[-1][2] < 0
    kinds = [r[4] % 4 == 0 and (r[4] >> 32) == (r[4] & 0xFFFFFFFF) and (r[3] & 0xFFFFFFFF) % 4 == 0
             for r in K.wprep_table("all, listed order")["wc"].seg_rows]
    assert any(kinds) and not all(kinds)                                # vec and scalar in one table


@pytest.mark.parametrize("Kc", K.PROBE_K)
def test_probe_oracle_matches_torch(Kc):
    for C in K.PROBE_C:
        for B in K.PROBE_B:
            x, W, b, y = K.probe_inputs(Kc, C, B)
            ref = O.classifier(x, W, b, y)
            v = ref["valid"]
            xd, Wd, bd = (t.to(F64).requires_grad_(True) for t in (x, W, b))
            z = F.linear(xd, Wd, bd)
            assert torch.equal(z.detach(), ref["z"])
            if v.any():
                rows = F.cross_entropy(z[v], y[v], reduction="none")
                assert torch.allclose(rows.detach(), ref["rowstat"][v, 0], rtol=1e-13, atol=1e-13)
                (dzt,) = torch.autograd.grad(rows.sum() / B, z)
                assert torch.allclose(dzt[v], ref["dz"][v], rtol=0, atol=1e-12)
            assert torch.allclose(ref["dz"][~v], torch.softmax(z.detach(), 1)[~v] / B, rtol=0, atol=1e-12)
            top = z.detach().topk(min(5, C), 1).values
            zl = z.detach().gather(1, y.clamp(0, C - 1)[:, None])
            assert torch.equal(ref["rowstat"][:, 1] == 1, v & (zl[:, 0] >= top[:, 0]))
            assert torch.equal(ref["rowstat"][:, 2] == 1, v & (zl[:, 0] >= top[:, -1]))


@pytest.mark.parametrize("C,Kc,B,first,wd", K.SGD_CASES)
def test_sgd_oracle_matches_hand_written_step(C, Kc, B, first, wd):
    d = K.sgd_inputs(C, Kc, B)
    h = K.sgd_hyper(C, first, wd)
    ref = O.sgd_step(d["x"], d["dz"], d["W"], d["b"], d["bufW"], d["bufb"], h["lr"], h["mom"], wd, first)
    W, b = d["W"].to(F64).requires_grad_(True), d["b"].to(F64).requires_grad_(True)
    (F.linear(d["x"].to(F64), W, b) * d["dz"].to(F64)).sum().backward()
    for prm, buf, n in ((W, d["bufW"], "W"), (b, d["bufb"], "b")):
        g = prm.grad + wd * prm.detach()
        nb = g.clone() if first else h["mom"] * buf.to(F64) + g
        assert torch.equal(nb, ref[f"buf{n}"]) and torch.equal(prm.detach() - h["lr"] * nb, ref[n])
    n4 = [c * k // 4 for c, k in K.SGD_SHAPES]           # below, at and above a multiple of the block
    assert any(n < 256 for n in n4) and any(n % 256 == 0 for n in n4) and any(n > 256 and n % 256 for n in n4)


# ------------------------------------------------------------------ the twins, and the guards --

@pytest.mark.parametrize("name", list(K.POOL_CASES))
def test_pool_twin(twin, name):
    K.check_pool(twin, name, {}, {})


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_pool_twin_grid_stride(twin, which):
    K.check_pool_grid(twin, which)


@pytest.mark.parametrize("name", list(K.WPREP_TABLES))
def test_wprep_twin(twin, name):
    gaps = K.check_wprep(twin, name)
    if name.startswith("all"):
        assert gaps > 0, "no alignment gap in the table: nothing shows a write between the slices"


@pytest.mark.parametrize("rows,Cp,C", K.UNPAD_CASES)
def test_unpad_add_twin(twin, rows, Cp, C):
    K.check_unpad_add(twin, rows, Cp, C)


@pytest.mark.parametrize("Kc", K.PROBE_K)
def test_probe_twin_exact(twin, Kc):
    for C in K.PROBE_C:
        for B in K.PROBE_B:
            K.check_probe_fwd_exact(twin, Kc, C, B, {})


@pytest.mark.parametrize("C,Kc,B,first,wd", K.SGD_CASES)
def test_sgd_twin_exact(twin, C, Kc, B, first, wd):
    K.check_sgd_exact(twin, C, Kc, B, first, wd)


@pytest.mark.parametrize("Kc", K.PROBE_WIDE_K)
def test_probe_twin_wide(twin, Kc):
    stats = {}
    for C, B in K.PROBE_WIDE_CB:
        K.check_probe_wide(twin, Kc, C, B, stats)
        K.check_sgd_wide(twin, Kc, C, B, stats)
    assert max(v for n, v in stats.items() if n.startswith("sgd")) <= 1.0


def test_sweep_and_eval_twin(twin):
    K.check_sweep(twin)
    K.check_eval_untouched(twin, 256, 65, 5)


# ------------------------------------------------------------------ the deliberate defects -----

@pytest.mark.parametrize("name", K.DEFECTS)
def test_defect_is_caught(name):
    check = K.DEFECT_CASES[name]
    check(K.TwinImpl())                                    # the case passes without the defect
    with pytest.raises(AssertionError):
        check(K.TwinImpl([name]))


def test_guards_were_exercised():
    """Runs last in this file: every exactness claim met its guard above, with room to spare."""
    for d in (K.pool_inputs(n) for n in K.POOL_CASES):
        K.guard_pool(d)
    w = K.GUARD.worst
    assert w["pool Σ|dy|"] < 2.0 ** 8 and w.get("logits", 0) < 2.0 ** 24 and w.get("sgd W", 0) < 2.0 ** 24
