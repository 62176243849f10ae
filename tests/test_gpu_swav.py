"""The SwAV kernels (csrc/kernels/swav.hip) on the GPU, stage by stage against fp64, so that no bound
is composed through the chain: every stage's reference is evaluated in fp64 on the kernel's OWN inputs
to that stage (its zhat and C, its S, its r, its u and c, its dS and dzhat).

u = 2^-24 (headgemm_checks.U); "1.01" covers second-order terms. All bounds are derived but two constants:

exp/log The kernels use __expf / __logf. No ROCm math document on the build machine states their
        error, so it is MEASURED: tools/explog_probe evaluates the intrinsics (a stand-alone kernel
        built with swav.hip's flags) on the fp32 arguments the kernels form from their own S at the four
        shapes below, (S − 1)·fp32(1/ε) (|x| <= 30.3), (S − max)·fp32(1/τ) (|x| <= 9.9) and Z (log Z in
        [1.7, 5.4]), against fp64 of the same fp32 argument. The error grows with the argument (it is
        multiplied by log2(e) in fp32), so it is modelled as __expf(x) = exp(x)(1 + δ), |δ| <= K_EXP·(1 +
        |x|)·u and __logf(l) = log l + ε, |ε| <= K_LOG·(1 + |log l|)·u. Worst seen on an MI355X: |δ| =
        1.1862·(1 + |x|)·u (28.8 u at most) and |ε| = 1.8355·(1 + |log l|)·u. Twice that is allowed:
        K_EXP = 2.38, K_LOG = 3.68 (margin 2.0; per shape in profiles/swav.txt). The argument is charged
        separately: x = fl(fl(s − 1)·fp32(1/ε)) resp. fl(fl(s − max)·fp32(1/τ)) carries two roundings,
        2u·|x| relative on the value (|x| <= 40 resp. 20). Together e(x) = (K_EXP·(1 + |x|) + 2|x|)·u.
prep    Σz² is an fp64 sum; rn = fp32(1/max(‖z‖, 1e-12)): u·rn. ẑ = fl(z·rn): 2u·|ẑ|, and so is C's row.
GEMMs   |err| <= (ε_p + R·u + ε_s)·Σ|a||b|, the bound of test_gpu_vicreg.py: ε_p = 2^-16 the per-product
        constant of hi·hi + hi·lo + lo·hi, R the reduction length, ε_s the fp32 roundings outside the
        MFMA chain: none for S and dẑ, u for dC (the factor g). Padding columns of S and dS: exactly 0.
first r a tile's column sum adds 64 values E·(1 + e) in fp32: 8 in a lane, 2 shuffles, 1 LDS add, 10
        additions of non-negative terms: 1.01·(ΣE·e + 10u·ΣE) for the fp64 sum of the partial rows.
rowsum  T − 1 fp32 additions of non-negative terms: (T − 1)·u·r against the fp64 sum of its partials.
u       fl(1/fl(K·r)) with a correctly rounded division: 2u·u_k.
c       Σ_k fl(E·u_k) in fp64, rounded once; against Σ E·u* with u* = 1/(K·r) in fp64: a term is off by
        e + 2u + u: 1.01·Σ_k E·u*·(e + 3u) + u·c.
next r  v_b = fl(1/fl(N·c_b)) from the kernel's c (2u), a term fl(E·v_b) one more, the strip's fp64 sum
        rounded once: 1.01·Σ_b E·v*·(e + 3u) + u·r for the fp64 sum of the partial rows.
q, Σq   q = fl(fl(u_k·E)·fl(1/c_b)): e_q = e + 3u relative to q* = u_k·E/c_b of the kernel's u and c.
        Σ_k q in fp64, rounded once: Σ q*·e_q + u. The kernel's c is itself Σ_k E·u_k within Σ q*·(e + u) + u
        (above, its own u), so |Σ_k q − 1| <= 1.01·(Σ_k q*·(2e + 4u) + 2u).
p, logp Z = Σ exp(x) in fp64, rounded: e_Z = Σ p*·e + u relative. p = fl(exp·fl(1/Z)): e_p = e + e_Z + 2u.
        log p = fl(x − __logf(Z)): |Δ| <= 2u|x| + K_LOG·(1 + |log Z|)·u + e_Z + u·|log p| =: a_lp.
loss    a row term Σ q_2·log p_1 + q_1·log p_2 in fp64: Σ q*·(e_q·|log p*| + a_lp), both orders; the sum
        over rows in fp64, divided and rounded: 1.01·that / (2N) + u·|L|.
dS      fl(fl(fl(p_1·Σq_2) − q_2)·s), s = fp32(1/(2Nτ)): 1.01·s·(p*Σq*·(e_p + e_Σq + u) + q*·e_q + u·|p*Σq* −
        q*|) + u·|dS|, e_Σq = Σ q*·e_q + u.
dz      fl(fl(dẑ − ẑ·t)·fl(g·rn)), t = fp32 of the fp64 dot product: 4u·(|dẑ| + |ẑ|·Σ|ẑ·dẑ|)·|g·rn|.

End to end the tolerances are set as test_gpu_vicreg.py sets them (1e-4 of the loss, 1e-3 of the largest
gradient element), not composed from the stage bounds: the codes q pass through three iterations whose
errors the stage tests bound one at a time.
"""
import pytest
import torch
import torch.nn.functional as F

import headgemm_checks as CK
from aux_oracle import f32_value

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = CK.U
EPS_P = 2.0 ** -16
K_EXP, K_LOG = 2.38, 3.68       # twice the worst measured (docstring)
EPS, TEMP, ITERS = 0.05, 0.1, 3
IE, IT = f32_value(1 / EPS), f32_value(1 / TEMP)
SHAPES = [(8, 64, 48), (40, 128, 200), (264, 192, 1000), (64, 64, 3000)]
WORST = CK.Worst()


def inputs(N, D, K, seed=0):
    """z: row norms spread over two decades; C random and unnormalised."""
    gen = torch.Generator().manual_seed(seed + 31 * N + D + K)
    z = [torch.randn(N, D, generator=gen, dtype=F64) * 10.0 ** (2 * torch.rand(N, 1, generator=gen, dtype=F64) - 1)
         for _ in range(2)]
    z[1] = z[1] + 0.5 * z[0]
    C = torch.randn(K, D, generator=gen, dtype=F64) * (0.5 + 1.5 * torch.rand(K, 1, generator=gen, dtype=F64))
    return z[0].float(), z[1].float(), C.float()


_CASE = {}


def case(N, D, K, dev):
    """The kernels' stage outputs (fp64 CPU tensors), computed once per shape."""
    if (N, D, K) not in _CASE:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require()
        z1, z2, C0 = (t.to(dev) for t in inputs(N, D, K))
        C = C0.clone()
        zhat, rnorm = m.swav_prep(z1, z2, C)
        S, part = m.swav_scores(zhat, C, EPS)
        o = dict(z1=z1, z2=z2, C0=C0, C=C, zhat=zhat, rnorm=rnorm, S=S)
        for it in range(ITERS):
            o[f"part{it}"] = part
            o[f"r{it}"] = r = m.swav_rowsum(part)
            o[f"u{it}"], o[f"c{it}"] = m.swav_sinkhorn(S, r, EPS, True)
            if it + 1 < ITERS:
                part = m.swav_sinkhorn(S, r, EPS, False)[0]
        u, c = o[f"u{ITERS - 1}"], o[f"c{ITERS - 1}"]
        o["loss"], o["dS"], o["qsum"] = m.swav_loss_grad(S, u, c, EPS, TEMP)
        g = torch.tensor([1.7], device=dev)
        o["dz"], o["dC"], o["dzhat"] = m.swav_bwd(zhat, rnorm, C, o["dS"], g, False)
        o["dC_frozen"] = m.swav_bwd(zhat, rnorm, C, o["dS"], g, True)[1]
        torch.cuda.synchronize()
        _CASE[N, D, K] = {k: v.cpu().to(F64) for k, v in o.items()}
    return _CASE[N, D, K]


def exp_err(x):
    return (K_EXP * (1 + x.abs()) + 2 * x.abs()) * U


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_prep_and_scores(gpu, N, D, K):
    c = case(N, D, K, gpu)
    ctx = f"[N={N} D={D} K={K}]"
    z = torch.cat([c["z1"], c["z2"]])
    rn = 1 / z.norm(dim=1)
    CK.within(WORST, "rnorm", c["rnorm"], rn, U * rn, ctx)
    CK.within(WORST, "zhat", c["zhat"], z * rn[:, None], 2.02 * U * (z * rn[:, None]).abs(), ctx)
    Cn = F.normalize(c["C0"], dim=1)
    CK.within(WORST, "C", c["C"], Cn, 2.02 * U * Cn.abs(), ctx)
    S = c["S"]
    assert S.shape == (2 * N, -(-K // 64) * 64) and not S[:, K:].any(), f"{ctx} padding of S"
    CK.within(WORST, "S", S[:, :K], c["zhat"] @ c["C"].t(), (EPS_P + D * U) * (c["zhat"].abs() @ c["C"].abs().t()), ctx)
    x = (S[:, :K] - 1) * IE
    E = x.exp()
    assert c["part0"].shape == (2, -(-N // 64), K)
    for v in range(2):
        Ev, ev = E[v * N:(v + 1) * N], exp_err(x[v * N:(v + 1) * N])
        CK.within(WORST, "r0", c["part0"][v].sum(0), Ev.sum(0), 1.01 * ((Ev * ev).sum(0) + 10 * U * Ev.sum(0)), ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_sinkhorn(gpu, N, D, K):
    c = case(N, D, K, gpu)
    ctx = f"[N={N} D={D} K={K}]"
    x = (c["S"][:, :K] - 1) * IE
    E, e = x.exp().view(2, N, K), exp_err(x).view(2, N, K)
    for it in range(ITERS):
        part, r = c[f"part{it}"], c[f"r{it}"]
        CK.within(WORST, "rowsum", r, part.sum(1), (part.shape[1] - 1) * U * part.sum(1) + 1e-300, ctx)
        us = 1 / (K * r)
        CK.within(WORST, "u", c[f"u{it}"], us, 2 * U * us, ctx)
        cs = (E * us[:, None, :]).sum(2)
        B = 1.01 * (E * us[:, None, :] * (e + 3 * U)).sum(2) + U * cs
        CK.within(WORST, "c", c[f"c{it}"], cs.reshape(-1), B.reshape(-1), ctx)
        if it + 1 < ITERS:
            vs = 1 / (N * c[f"c{it}"].view(2, N, 1))
            rs = (E * vs).sum(1)
            nxt = c[f"part{it + 1}"]
            assert nxt.shape == (2, -(-N // 16), K)
            CK.within(WORST, "next_r", nxt.sum(1), rs, 1.01 * (E * vs * (e + 3 * U)).sum(1) + U * rs, ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_loss_grad(gpu, N, D, K):
    c = case(N, D, K, gpu)
    ctx = f"[N={N} D={D} K={K}]"
    S = c["S"][:, :K]
    x = (S - 1) * IE
    e_q = exp_err(x) + 3 * U
    q = c[f"u{ITERS - 1}"].repeat_interleave(N, 0) * x.exp() / c[f"c{ITERS - 1}"][:, None]
    sq = q.sum(1)
    e_sq = (q * e_q).sum(1) / sq + U
    CK.within(WORST, "qsum", c["qsum"], sq, sq * e_sq, ctx)
    CK.within(WORST, "qsum=1", c["qsum"], torch.ones(2 * N, dtype=F64),
              1.01 * ((q * (2 * exp_err(x) + 4 * U)).sum(1) + 2 * U), ctx)
    xp = (S - S.max(1, keepdim=True).values) * IT
    Z = xp.exp().sum(1, keepdim=True)
    p, logp = xp.exp() / Z, xp - Z.log()
    e_Z = (p * exp_err(xp)).sum(1, keepdim=True) + U
    e_p = exp_err(xp) + e_Z + 2 * U
    a_lp = 2 * U * xp.abs() + K_LOG * (1 + Z.log().abs()) * U + e_Z + U * logp.abs()
    swap = torch.cat([torch.arange(N, 2 * N), torch.arange(N)])     # the other view's rows
    qo, e_qo, sqo, e_sqo = q[swap], e_q[swap], sq[swap, None], e_sq[swap, None]
    loss = -(qo * logp).sum() / (2 * N)
    B = 1.01 * (qo * (e_qo * logp.abs() + a_lp)).sum() / (2 * N) + U * loss.abs()
    CK.within(WORST, "loss", c["loss"], loss.reshape(1), B.reshape(1), ctx)
    s = f32_value(1 / (2 * N * TEMP))
    dS = (p * sqo - qo) * s
    B = 1.01 * s * (p * sqo * (e_p + e_sqo + U) + qo * e_qo + U * (p * sqo - qo).abs()) + U * dS.abs()
    assert not c["dS"][:, K:].any(), f"{ctx} padding of dS"
    CK.within(WORST, "dS", c["dS"][:, :K], dS, B, ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_backward(gpu, N, D, K):
    c = case(N, D, K, gpu)
    ctx = f"[N={N} D={D} K={K}]"
    g = f32_value(1.7)
    dS, C, zh, dh = c["dS"], c["C"], c["zhat"], c["dzhat"]
    Kp = dS.shape[1]
    CK.within(WORST, "dzhat", dh, dS[:, :K] @ C, (EPS_P + Kp * U) * (dS[:, :K].abs() @ C.abs()), ctx)
    CK.within(WORST, "dC", c["dC"], g * (dS[:, :K].t() @ zh),
              (EPS_P + 2 * N * U + U) * g * (dS[:, :K].abs().t() @ zh.abs()), ctx)
    assert c["dC_frozen"].shape == (K, D) and not c["dC_frozen"].any()
    gr = g * c["rnorm"][:, None]
    dz = gr * (dh - zh * (zh * dh).sum(1, keepdim=True))
    CK.within(WORST, "dz", c["dz"], dz, 4 * U * (dh.abs() + zh.abs() * (zh * dh).abs().sum(1, keepdim=True)) * gr, ctx)
    print(ctx, WORST.report())


def test_module_end_to_end(gpu):
    """SwAVLoss (native) against fp64 autograd of swav_reference on the fp64-normalised prototypes."""
    from simclr_pytorch_distributed_amd.losses import SwAVLoss, swav_reference
    N, D, K = 40, 128, 200
    z1, z2, C0 = inputs(N, D, K, seed=7)
    C = torch.nn.Parameter(C0.to(gpu))
    feats = torch.cat([z1, z2]).to(gpu).requires_grad_(True)
    loss = SwAVLoss(C, EPS, TEMP, ITERS, backend="native")(feats)
    (1.7 * loss).backward()
    a, b = z1.to(F64).requires_grad_(True), z2.to(F64).requires_grad_(True)
    Cr = F.normalize(C0.to(F64), dim=1).requires_grad_(True)
    ref = swav_reference(a, b, Cr, EPS, TEMP, ITERS)
    (1.7 * ref).backward()
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    assert (C.detach().cpu().to(F64) - Cr.detach()).abs().max() <= 4 * U
    for name, got, want in (("dz", feats.grad, torch.cat([a.grad, b.grad])), ("dC", C.grad, Cr.grad)):
        err = (got.cpu().to(F64) - want).abs().max().item()
        print(f"e2e {name} err/max {err / want.abs().max().item():.3g}")
        assert err <= 1e-3 * want.abs().max().item(), name


def test_bit_identical_runs(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    z1, z2, C0 = (t.to(gpu) for t in inputs(264, 192, 1000))
    g = torch.ones(1, device=gpu)
    outs = []
    for _ in range(2):
        C = C0.clone()
        loss, zhat, rnorm, dS = m.swav_fwd(z1, z2, C, EPS, TEMP, ITERS)
        outs.append([loss, zhat, rnorm, dS, C, *m.swav_bwd(zhat, rnorm, C, dS, g, False)])
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_engine_step(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.ops import swav
    norms = []
    native = swav.swav_loss

    def spy(z1, z2, C, *a):
        before = C.detach().norm(dim=1).clone()     # step 2: the rows as weight decay left them
        out = native(z1, z2, C, *a)
        norms.append((C.detach().norm(dim=1).clone(), a[-1], before))     # after swav_prep, before the update
        return out

    monkeypatch.setattr(swav, "swav_loss", spy)
    opt = parse_pretrain(["--method", "SwAV", "--swav_prototypes", "200", "--swav_freeze_iters", "1", "--model",
                          "resnet18", "--synthetic", "--synthetic_size", "64", "--batch_size", "32", "--feat_dim", "128",
                          "--max_steps", "2", "--backend", "native", "--work_dir", str(tmp_path)], make_dirs=False)
    eng = PretrainEngine(opt)
    w = eng.model.prototypes.weight
    assert w.shape == (200, 128) and w.data_ptr() == eng.flat.flat[eng.flat.offsets[eng.flat.names.index(
        "prototypes.weight")]:].data_ptr()
    dirs = [F.normalize(w.detach().clone(), dim=1)]
    for it in range(opt.max_steps):
        st = eng.train_step(torch.arange(32 * it, 32 * it + 32, device=gpu), 1, it, 2)
        assert torch.isfinite(st["loss_local"]).item()
        dirs.append(F.normalize(w.detach().clone(), dim=1))
    assert [f for _, f, _ in norms] == [True, False]
    assert all((n - 1).abs().max().item() <= 4 * U < (b - 1).abs().min().item() for n, _, b in norms)
    assert (dirs[1] - dirs[0]).abs().max().item() <= 1e-6 < (dirs[2] - dirs[1]).abs().max().item()
