"""CPU proof for the contrastive-loss oracle tests: the fp64 oracle of tests/supcon_oracle.py is
right (against fp64 autograd of the dense formulation and the package's CPU path), the bounds of
tests/supcon_checks.py hold for a correct fp32 evaluation with 2x room in two accumulation
orders, every deliberate defect lies outside them, and every case sits on the path it is
named for. No GPU."""
import numpy as np
import pytest
import torch

import supcon_checks as K
import supcon_oracle as O

F64 = torch.float64


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


# ---------------------------------------------------------------- the oracle itself -----------

def _dense_autograd(feats, key, mode, tau, tau_base):
    """The dense formulation (logits − max, exp·logits_mask, mask·log_prob) with masks built here;
    A and C are separate leaves so that dA and dC come out separately."""
    bsz, nv, _ = feats.shape
    C = torch.cat(torch.unbind(feats, 1), 0).clone().requires_grad_(True)
    na = bsz * nv if mode == "all" else bsz
    A = C.detach()[:na].clone().requires_grad_(True)
    logits = A @ C.t() / tau
    logits = logits - logits.max(1, keepdim=True).values.detach()
    same = (key[:, None] == key[None, :]).to(F64).repeat(na // bsz, nv)
    logits_mask = torch.ones_like(same)
    logits_mask[torch.arange(na), torch.arange(na)] = 0
    mask = same * logits_mask
    log_prob = logits - torch.log((torch.exp(logits) * logits_mask).sum(1, keepdim=True))
    rows = -(tau / tau_base) * (mask * log_prob).sum(1) / mask.sum(1)
    loss = rows.mean()
    (loss * 1.7).backward()
    return loss.detach(), rows.detach(), A.grad, C.grad


# SimCLR keys with one view have no positives (the dense form is NaN there): not in the table
@pytest.mark.parametrize("mode,supcon,nv", [(m, s, v) for m in ("one", "all") for s in (False, True)
                                            for v in (1, 2, 3, 4) if s or v > 1])
def test_exact_equals_dense_autograd(mode, supcon, nv):
    g = torch.Generator().manual_seed(nv)
    bsz, D, tau = 12, 16, 0.1
    feats = torch.nn.functional.normalize(torch.randn(bsz, nv, D, generator=g, dtype=F64), dim=-1)
    key = torch.arange(bsz) % 4 if supcon else torch.arange(bsz)
    loss, rows, dA, dC = _dense_autograd(feats, key, mode, tau, 0.07)
    C = torch.cat(torch.unbind(feats, 1), 0)
    na = bsz * nv if mode == "all" else bsz
    ck = key.repeat(nv)
    e = O.exact(C[:na], C, torch.arange(na), ck[:na], ck, tau, 0.07, 1.0 / na, 1.7)
    assert _rel(e["loss"], loss) <= 1e-12 and _rel(e["rows"], rows) <= 1e-12
    assert _rel(e["dA"], dA) <= 1e-12 and _rel(e["dC"], dC) <= 1e-12


@pytest.mark.parametrize("name", ["nopos_some", "nopos_all", "own_r2_one_SupCon", "self_perm", "views3"])
def test_exact_equals_package_cpu_path(name):
    """supcon_rows_reference in fp64, the no-positive convention included."""
    from simclr_pytorch_distributed_amd.losses.supcon import supcon_rows_reference
    c = K.cases()[name]
    A, C = c.A.double().requires_grad_(True), c.C.double().requires_grad_(True)
    rows = supcon_rows_reference(A, C, c.self_idx, c.akey, c.ckey, c.tau, K.TAU_BASE)
    (c.scale * rows.sum() * c.g).backward()
    e = O.exact(*c.args(), c.g)
    assert (rows.detach() - e["rows"]).abs().max() <= 1e-12 * max(1.0, e["rows"].abs().max().item())
    assert (rows.detach()[~e["has"]] == 0).all()
    scale = max(e["dC"].abs().max().item(), 1e-30)
    assert (A.grad - e["dA"]).abs().max() <= 1e-12 * scale and (C.grad - e["dC"]).abs().max() <= 1e-12 * scale


def test_bf16_rne_matches_integer_rounding():
    """x.bfloat16() is the integer-arithmetic round-to-nearest-even, at exact ties (both
    parities), just off them, subnormals, negative zero and the lo parts of a split."""
    def f(bits):
        return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
    ties = f([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F818001, 0x3F817FFF, 0xBF808000, 0xBF818000,
              0x00008000, 0x00018000, 0x00000001, 0x00007FFF, 0x80000000, 0x00000000, 0x7F7E8000, 0x007F8000])
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4096, generator=g) * 10.0 ** torch.randint(-42, 4, (4096,), generator=g)
    lo = x - O.bf16_rne(x)                    # lo parts, subnormal ones among them
    assert (lo.abs() < 2.0 ** -126).any() and (lo != 0).any()
    for t in (ties, x, lo):
        a, b = O.bf16_rne(t), O.bf16_rne_int(t)
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))
    assert O.bf16_rne(f([0x3F808000])).item() == 1.0 and O.bf16_rne(f([0x3F818000])).item() == 1.015625
    nz = O.bf16_rne(f([0x80000000]))
    assert nz.item() == 0 and np.signbit(nz.numpy())[0]
    hi, lo = O.split(x)
    assert torch.equal((x - hi).double(), x.double() - hi.double())      # x − hi is exact in fp32


def test_split_model_inside_split_bound_and_sharp():
    """The header's "~2^-16" per logit: |a_lo·c_lo| and the split remainders; some logit of some
    case uses at least a tenth of the bound."""
    worst = 0.0
    for name in K.case_names():
        c = K.cases()[name]
        e, s = O.exact(*c.args(), c.g), O.split_model(*c.args(), c.g)
        B = O.split_bound(c.A, c.C, c.tau)
        err = (e["logits"] - s["logits"]).abs()
        assert (err <= B).all(), name
        # lse is 1-Lipschitz in the logits (max norm)
        assert ((e["lse"] - s["lse"]).abs() <= torch.where(e["not_self"], B, torch.zeros((), dtype=F64)).max(1).values
                * (1 + 1e-9) + 1e-15).all(), name
        assert (B <= 3.1 * 2.0 ** -18 * (c.A.double().abs() @ c.C.double().abs().t()) / c.tau).all(), name
        worst = max(worst, (err / B).max().item())
    print(f"split_model vs exact: largest logit error / bound = {worst:.3f}")
    assert worst >= 0.1


# ---------------------------------------------------------------- twins against the bounds ----

@pytest.fixture(scope="module")
def twin_ratios():
    out = {}
    for rev in (False, True):
        tw = K.TwinImpl(reverse=rev)
        for name in K.case_names():
            st = {}
            K.check_case(tw, name, st)          # asserts ratio <= 1 and the exact-zero conditions
            out[(rev, name)] = st
    return out


@pytest.mark.parametrize("reverse", [False, True])
def test_twin_within_half_of_every_bound(twin_ratios, reverse):
    worst = {}
    for (rev, name), st in twin_ratios.items():
        if rev == reverse:
            for k, v in st.items():
                assert v <= 0.5, (name, k, v)
                worst[k] = max(worst.get(k, 0.0), v)
    for k in sorted(worst):
        print(f"twin (reverse={reverse}) {k}: largest error / bound = {worst[k]:.4f}")


@pytest.mark.parametrize("wrong", sorted(K.WRONG))
def test_wrong_twin_is_outside(wrong):
    tw = K.TwinImpl(wrong=wrong)
    for name in K.WRONG[wrong]:
        r = K.check_case(tw, name, strict=False)
        print(f"{wrong} at {name}: error / bound = {r:.4g}")
        assert r > 4.0, (wrong, name, r)


def test_twin_exp_is_the_exp2_form():
    x = torch.linspace(-80, 0, 1001)
    assert torch.equal(K._exp(x), torch.exp2(x * torch.tensor(1.4426950408889634)))
    assert K._exp(torch.tensor(float("-inf"))).item() == 0 and K._exp(torch.tensor(0.0)).item() == 1


# ---------------------------------------------------------------- cases on their paths --------

def test_split_mirrors():
    assert K.fwd_geometry(1500, 1500) == (22, 96) and K.empty_fwd_splits(1500, 1500) == 6
    assert K.bwd_geometry(1500, 1500) == (16, 96)
    assert K.fwd_geometry(200, 200) == (4, 64) and K.fwd_geometry(1, 33) == (1, 64)
    assert K.fwd_split_ranges(65, 65) == [(0, 64), (64, 65)]
    assert K.bwd_geometry(96, 384) == (6, 64) and K.bwd_geometry(384, 96) == (2, 64)
    try:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require() if _ext.available() else None
    except Exception:  # noqa: BLE001
        m = None
    if m is not None and hasattr(m, "supcon_num_splits"):      # host-only query, no GPU needed
        for a, b in [(1, 33), (15, 65), (64, 64), (65, 65), (200, 200), (129, 257), (1500, 1500), (96, 384),
                     (384, 96), (1024, 8192), (8192, 1024), (40000, 64), (3, 1)]:
            assert m.supcon_num_splits(a, b) == K.pick_splits(a, b), (a, b)


def test_cases_sit_on_their_paths():
    f = {n: K.path_facts(K.cases()[n]) for n in K.case_names()}
    e = f["empty_splits"]
    assert (e["fwd_splits"], e["empty"], e["bwd_a"], e["bwd_c"]) == (22, 6, 16, 16)
    assert f["empty_splits_low"]["empty"] == 6
    assert float((K._model(K.cases()["empty_splits_low"])["max"]).max()) < -88.0
    assert f["edge_1x33_D64"]["last_tile"] == 1 and f["max_tail"]["last_tile"] == 1       # N ≡ 1 (mod 32)
    assert f["edge_65x65_D256"]["self_alone_in_split"] == 1          # split 1 of anchor 64: only its self row
    assert f["edge_15x65_D128"]["last_tile"] == 1 and K.cases()["edge_15x65_D128"].Na < 16
    assert K.cases()["edge_129x257_D64"].Na % 64 == 1 and K.cases()["edge_65x65_D256"].Na % 64 == 1
    s = f["self_place"]
    assert s["self_first_of_tile"] >= 2 and s["self_last_of_tile"] >= 2 and s["self_last_of_split"] >= 3
    assert s["self_last_row"] == 1
    p = K.cases()["self_perm"].self_idx
    assert sorted(p.tolist()) == list(range(96)) and not torch.equal(p, torch.arange(96, dtype=torch.int32))
    assert f["nopos_all"]["no_pos"] == 65 and f["nopos_one"]["no_pos"] == 1 and 1 < f["nopos_some"]["no_pos"] < 70
    assert all(f[n]["no_pos"] == 0 for n in f if n.startswith(("own_", "views", "edge_", "max_", "g_")) or n == "dup")
    # row ownership: base r·96 (all) and the first 48 of it (one), from the production builder
    for r in (0, 2, 3):
        for method in ("SimCLR", "SupCon"):
            a, o = K.cases()[f"own_r{r}_all_{method}"], K.cases()[f"own_r{r}_one_{method}"]
            assert a.N == o.N == 384 and a.self_idx.tolist() == list(range(96 * r, 96 * r + 96))
            assert o.self_idx.tolist() == list(range(96 * r, 96 * r + 48))
    # the position of the maximum of anchor 0's row
    for name, where in (("max_first", 5), ("max_last", 90), ("max_tail", 96)):
        c = K.cases()[name]
        S = (c.A[0].double() @ c.C.double().t())
        S[0] = -2
        assert int(S.argmax()) == where and S[where] > 0.99 and S.topk(2).values[1] < 0.6
    c = K.cases()["max_last"]
    assert K.fwd_split_ranges(c.Na, c.N) == [(0, 64), (64, 96)]
    c = K.cases()["dup"]
    assert all(torch.equal(c.C[j], c.A[0]) for j in (10, 50, 96)) and int(c.self_idx[0]) == 0
    # every D in the forward, the two-output and the merged backward; every temperature
    assert {(c.D, c.same) for c in K.cases().values()} >= {(D, s) for D in (64, 128, 256) for s in (False, True)}
    assert {c.tau for c in K.cases().values()} == {0.5, 0.1, 0.07, 0.02}
    assert {c.g for c in K.cases().values()} == {1.7, 0.0, -0.6}
    assert all(n in K.cases() for names in K.WRONG.values() for n in names)
    assert all(n in K.cases() for n in K.REPEAT_CASES)


# ---------------------------------------------------------------- rank decomposition ----------

@pytest.mark.parametrize("mode", ["all", "one"])
@pytest.mark.parametrize("method", ["SimCLR", "SupCon"])
def test_rank_decomposition(mode, method):
    """W = 4: the rank-r row-form losses built from DistributedContrastiveLoss._indices add up to
    the whole-batch loss, and per-rank dC plus dA scattered to the owners to its gradient (fp64).
    tests/test_dist.py checks the same through real processes and fp32."""
    from simclr_pytorch_distributed_amd.losses.supcon import DistributedContrastiveLoss
    w, nv, b, D, tau = 4, 2, 6, 16, 0.1
    g = torch.Generator().manual_seed(3)
    n = w * nv * b
    C = torch.nn.functional.normalize(torch.randn(n, D, generator=g, dtype=F64), dim=1)
    labels = torch.randint(0, 5, (w * b,), generator=g) if method == "SupCon" else None
    crit = DistributedContrastiveLoss(method, tau, 0.07, contrast_mode=mode, n_views=nv, backend="torch")
    parts = [crit._indices(b, w, r, torch.device("cpu"), labels) for r in range(w)]
    ckey = parts[0][2]
    assert all(torch.equal(p[2], ckey) for p in parts)
    si_all = torch.cat([p[0] for p in parts])
    na = si_all.numel()
    whole = O.exact(C[si_all.long()], C, si_all, ckey[si_all.long()], ckey, tau, 0.07, 1.0 / na, 1.7)
    want = whole["dC"].clone()
    want.index_add_(0, si_all.long(), whole["dA"])
    loss, grad = torch.zeros((), dtype=F64), torch.zeros_like(C)
    for si, ak, ck in parts:
        e = O.exact(C[si.long()], C, si, ak, ck, tau, 0.07, 1.0 / na, 1.7)
        loss += e["loss"]
        grad += e["dC"]
        grad.index_add_(0, si.long(), e["dA"])
    assert abs(loss - whole["loss"]) <= 1e-12 * abs(whole["loss"])
    assert (grad - want).abs().max() <= 1e-12 * want.abs().max()
    if mode == "all":      # the gathered batch as one rank sees it when W = 1
        assert sorted(si_all.tolist()) == list(range(n))
