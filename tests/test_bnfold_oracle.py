"""CPU tests of the BN3 fold oracle (tests/bnfold_oracle.py) and of the cases, bounds, guard and
twin of tests/bnfold_checks.py: the folded formulas equal the unfolded definition in float64, the
coherent-rounding correction does what bnfold.hip claims, every exact case passes the guard, the
fp32 twin is bit-equal in the exact regime and within half of every wide bound, every deliberate
defect is caught at its named case, and every case takes the branch it is named for."""
import pytest
import torch

import bnfold_checks as K
import bnfold_oracle as O
from conv_oracle import rne_bf16

F64 = torch.float64


def _close(a, b, rel=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert (a - b).abs().max().item() <= rel * b.abs().max().clamp_min(1e-300).item(), (a - b).abs().max().item()


def _bn_case(rows, C=24, Kc=16, seed=0):
    """A real BN backward in fp64: y3 = a2·W3ᵀ, z = BN(y3), dz = dL/dz -> per-channel A, D, E of
    dy3 = A·dz + D·y3 + E."""
    g = torch.Generator().manual_seed(seed)
    a2 = torch.randn(rows, Kc, generator=g).clamp_min(0).bfloat16().to(F64)
    W = torch.randn(C, Kc, generator=g).bfloat16().to(F64)
    dz = torch.randn(rows, C, generator=g).bfloat16().to(F64) + 0.3
    gamma = (torch.rand(C, generator=g) + 0.5).to(F64)
    y3 = a2 @ W.T
    mu = y3.mean(0)
    inv = 1.0 / torch.sqrt(y3.var(0, unbiased=False) + 1e-5)
    A = gamma * inv
    D = -A * inv * inv * (dz * (y3 - mu)).mean(0)
    E = -A * dz.mean(0) - D * mu
    return dict(a2=a2, W=W, dz=dz, gamma=gamma, y3=y3, mu=mu, inv=inv, A=A, D=D, E=E)


def test_bn_coefficients_are_the_bn_backward():
    """The A, D, E of _bn_case against autograd, so that the tests below stand on a real BN."""
    c = _bn_case(40)
    y = c["y3"].clone().requires_grad_(True)
    z = torch.nn.functional.batch_norm(y, None, None, c["gamma"], torch.zeros_like(c["gamma"]), training=True,
                                       eps=1e-5)
    z.backward(c["dz"])
    _close(c["A"] * c["dz"] + c["D"] * c["y3"] + c["E"], y.grad, 1e-11)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_folded_equals_unfolded(seed):
    g = torch.Generator().manual_seed(seed)
    rows, C, Kc = 37, 11, 24
    A, D, E = (torch.randn(C, generator=g, dtype=F64) for _ in range(3))
    dz, a2 = torch.randn(rows, C, generator=g, dtype=F64), torch.randn(rows, Kc, generator=g, dtype=F64)
    W = torch.randn(C, Kc, generator=g, dtype=F64)
    u, f = O.unfolded(A, D, E, dz, a2, W), O.folded(A, D, E, dz, a2, W)
    _close(f["da2"], u["da2"])
    _close(f["dW"], u["dW"])
    _close(f["dzy"], u["dzy"])
    # the per-operation oracles are the same formulas
    coef = torch.cat([A, D, E])
    _close(O.prep_mx(coef, W)[0], f["Mx"])
    _close(O.wgrad(coef, f["G"], f["S"], f["cs"][None, :], W)[0], u["dW"])
    _close(O.rowdot(f["G"], W)[0], u["dzy"])
    _close(O.colsum(a2)[0], f["cs"])


@pytest.mark.parametrize("rows", [64, 256, 1000])
def test_coherent_correction(rows):
    """mean(dz) = −(E + D·μ)/A for the coefficients of a real BN backward, and the row sums of
    the folded da2 with bf16 Wd and Mx equal those of the true da2 with the correction and are
    off by rows·(the row-mean rounding error) without it."""
    c = _bn_case(rows)
    A, D, E, W, dz, a2 = (c[k] for k in ("A", "D", "E", "W", "dz", "a2"))
    C, Kc = W.shape
    coef = torch.cat([A, D, E])
    _close(O.mean_dz(coef, c["mu"], C), dz.mean(0), 1e-9)
    wd = rne_bf16(O.f32(A[:, None] * W)).T                 # [K][C], as stored
    mx_true, _ = O.prep_mx(coef, W)
    mx = rne_bf16(O.f32(mx_true))
    true_sum = O.unfolded(A, D, E, dz, a2, W)["da2"].sum(0)
    with_c = O.prep_bias(coef, W, c["mu"], a2.sum(0), rows, wd, mx)["b"]
    without = O.prep_bias(coef, W, None, None, rows, wd, mx)["b"]
    fold = (dz @ wd.T + a2 @ mx).sum(0)
    scale = (dz.abs() @ wd.T.abs() + a2 @ mx.abs()).sum(0).max().item()
    assert ((fold + rows * with_c) - true_sum).abs().max().item() <= 1e-12 * scale
    row_mean_err = dz.mean(0) @ (A[:, None] * W - wd.T) + (mx_true - mx) @ a2.mean(0)
    off = (fold + rows * without) - true_sum
    assert (off + rows * row_mean_err).abs().max().item() <= 1e-12 * scale
    assert (rows * row_mean_err).abs().max().item() >= 1e4 * 1e-12 * scale      # far above the noise: ∝ rows


# ---------------------------------------------------------------- guard, twin ----------------

TWIN = K.TwinImpl()


@pytest.mark.parametrize("name", list(K.PREP_CASES))
def test_twin_prep(name):
    K.check_prep(TWIN, name, "exact")           # runs the guard of the case
    stats = {}
    K.check_prep(TWIN, name, "wide", stats)
    assert stats["prep b"] <= 0.5, stats
    # Mx before its rounding against the fp32 bound itself
    d = K.prep_inputs(name, "wide")
    probe = {}
    K.twin_prep(K._np(d["coef"]), K._np(d["W"]), K._np(d["mu"]), K._np(d["cs"]), d["rows"],
                K.prep_layout(d["C"], d["K"], d["cat"]), probe=probe)
    ref, ref_abs = O.prep_mx(d["coef"], d["W"])
    err = (torch.from_numpy(probe["mx_fp32"]) - ref).abs()
    assert (err <= 0.5 * K.gamma(K.mx_depth(d["C"], d["K"])) * ref_abs).all()


def test_corr_case_exercises_both_corrections():
    d = K.prep_inputs("corr (256, 64)", "exact")
    mx, _ = O.prep_mx(d["coef"], d["W"])
    assert mx.abs().max() > 256 and (mx != rne_bf16(mx)).any()
    wd = O.prep_wd(d["coef"], d["W"])
    A = d["coef"][:256].to(F64)
    assert ((A[:, None] * d["W"].to(F64) - wd.T) != 0).any()
    full = O.prep_bias(d["coef"], d["W"], d["mu"], d["cs"], d["rows"], wd, rne_bf16(mx))["b"]
    for mu, cs in ((None, d["cs"]), (d["mu"], None)):
        part = O.prep_bias(d["coef"], d["W"], mu, cs, d["rows"], wd, rne_bf16(mx))["b"]
        assert (part != full).any()


@pytest.mark.parametrize("Kc,rows", K.COLSUM_CASES)
def test_twin_colsum(Kc, rows):
    K.check_colsum(TWIN, Kc, rows, "exact")
    stats = {}
    K.check_colsum(TWIN, Kc, rows, "wide", stats)
    assert max(stats.values()) <= 0.5, stats


@pytest.mark.parametrize("C,Kc,ncs,acc", K.WGRAD_CASES)
def test_twin_wgrad(C, Kc, ncs, acc):
    K.check_wgrad(TWIN, C, Kc, ncs, acc, "exact")
    stats = {}
    K.check_wgrad(TWIN, C, Kc, ncs, acc, "wide", stats)
    assert stats["wgrad"] <= 0.5, stats


@pytest.mark.parametrize("C,Kc,ns", K.ROWDOT_CASES)
def test_twin_rowdot(C, Kc, ns):
    stats = {}
    for kind in K.ROWDOT_KINDS:
        K.check_rowdot(TWIN, C, Kc, ns, kind, stats)
    assert max(stats.values()) <= 0.5, stats


# ---------------------------------------------------------------- defects --------------------

def test_defect_tables_cover_every_defect():
    assert len(K.DEFECTS) >= 10 and set(K.DEFECT_CASES) == set(K.DEFECTS)
    assert set(K.DEFECT_CASES_WIDE) <= set(K.DEFECTS)


@pytest.mark.parametrize("name", K.DEFECTS)
def test_defect_is_caught_exact(name):
    check, _ = K.DEFECT_CASES[name]
    check(TWIN, None)                                    # the case itself passes
    with pytest.raises(AssertionError):
        check(K.TwinImpl([name]), None)


@pytest.mark.parametrize("name", list(K.DEFECT_CASES_WIDE))
def test_defect_is_caught_wide(name):
    """By at least 4x the bound."""
    check, stat = K.DEFECT_CASES_WIDE[name]
    stats = {}
    with pytest.raises(AssertionError):
        check(K.TwinImpl([name]), stats)
    assert stats[stat] >= 4.0, stats


# ---------------------------------------------------------------- branches -------------------

def test_prep_cases_take_their_branches():
    path = {n: K.prep_path(p["C"], p["K"]) for n, p in K.PREP_CASES.items()}
    assert path["P > C (1, 8)"]["P"] == 128 > 1
    assert path["(7, 64) cat"]["P"] == 16 > 7
    assert path["production (256, 64)"] == dict(KW=64, P=16, k0_trips=1, gw=16, wd_strided=False, c_trips=1)
    assert path["production (512, 128)"] == dict(KW=128, P=8, k0_trips=1, gw=64, wd_strided=False, c_trips=1)
    big = path["C > 1024, Wd grid-stride (1030, 512)"]
    assert big["c_trips"] == 2 and big["gw"] == 256 and big["wd_strided"]
    assert path["P = 1 (64, 1024)"]["P"] == 1 and path["P = 1 (64, 1024)"]["k0_trips"] == 1
    assert path["two k0 trips (64, 2048)"]["k0_trips"] == 2 and path["two k0 trips (64, 2048)"]["KW"] == 1024
    assert path["largest C (8192, 8)"]["c_trips"] == 8 and K.prep_accepts(8192, 8)
    for n, p in K.PREP_CASES.items():
        assert K.prep_accepts(p["C"], p["K"]), n
        lay = K.prep_layout(p["C"], p["K"], p["cat"])
        assert K.prep_accepts(p["C"], p["K"], lay["arg_ldw"], lay["arg_ldm"]), n
    for n, (C, Kc, ldw, ldm) in K.PREP_REFUSED.items():
        assert not K.prep_accepts(C, Kc, ldw, ldm), n
    # the variants: mu and cs each absent and present, rows 0, A = 0, both layouts
    v = K.PREP_CASES
    assert {(p["mu"], p["cs"]) for p in v.values()} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(not p["rows"] for p in v.values()) and any(p["a0"] for p in v.values())
    assert {p["cat"] for p in v.values()} == {True, False}
    d = K.prep_inputs("(7, 64) A = 0", "wide")
    assert (d["coef"][:7] == 0).sum() == 2 and d["mu"] is not None


def test_colsum_cases_take_their_branches():
    S = K.COLSUM_STRIDE
    assert [n8 for Kc, n8 in K.COLSUM_CASES if Kc == 8] == K.COLSUM_N8
    assert K.colsum_trips(1) == ((0, 0), (0, 1))                 # one thread, every other idle
    assert K.colsum_trips(255) == ((0, 0), (0, 1))
    assert K.colsum_trips(S - 1) == ((0, 0), (0, 1))             # one full trip but for the last thread
    assert K.colsum_trips(S + 3) == ((0, 0), (1, 2))
    assert K.colsum_trips(5 * S + 77) == ((1, 1), (1, 2))        # the unrolled loop, then one or two of the tail
    assert {Kc for Kc, _ in K.COLSUM_CASES} == {8, 64, 128, 2048}
    for Kc, rows in K.COLSUM_CASES:
        assert K.colsum_accepts(Kc) and rows * Kc * 2 <= 11 * 2 ** 20
    assert K.colsum_trips(2561 * 2048 // 8)[0] == (1, 1) and (2048, 2561) in K.COLSUM_CASES
    assert not any(K.colsum_accepts(Kc) for Kc in K.COLSUM_REFUSED)


def test_wgrad_and_rowdot_cases_take_their_branches():
    blocks = {Kc: K.wgrad_block(Kc) for _, Kc, _, _ in K.WGRAD_CASES}
    assert blocks == {8: 64, 72: 128, 64: 64, 320: 256, 8192: 256}
    # K < block (idle lanes), K == block, K > block (the k loop runs 2 and 32 times)
    assert 72 < blocks[72] and 64 == blocks[64] and 320 > blocks[320] and 8192 == 32 * blocks[8192]
    assert {n for _, _, n, _ in K.WGRAD_CASES} == {1, 3, 512}
    assert {a for _, _, _, a in K.WGRAD_CASES} == {0, 1}
    assert {(C, Kc) for C, Kc, _, _ in K.WGRAD_CASES} == {(1, 8), (5, 72), (256, 64), (3, 320), (2, 8192)}
    assert {(C, Kc) for C, Kc, _ in K.ROWDOT_CASES} == {(1, 8), (7, 100), (512, 128)}
    assert {ns for _, _, ns in K.ROWDOT_CASES} == {2, 3}
    # K = 8: 56 idle lanes; K = 100: a second, ragged trip; K = 128: two full trips
    assert 8 < 64 < 100 < 128
