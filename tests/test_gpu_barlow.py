"""The Barlow Twins kernels (csrc/kernels/barlow.hip) on the GPU, stage by stage against fp64, so
that no bound is composed through the chain: every stage's reference is evaluated in fp64 on the
kernel's OWN inputs to that stage (its fp32 stats, its C, its G and r).

u = 2^-24. The bounds are derived here, none is measured (worst error / bound per stage on an
MI355X: profiles/barlow.txt).

stats   The sums run in fp64 (error (N + 4)·2^-52 of Σ|z| resp. Σz²), then one rounding to fp32:
        |Δμ| <= u·|μ| + (N + 4)·2^-52·mean|z|;  |Δrstd| <= rstd·(u + (N + 4)·2^-52·mean z² / (var + ε))
        (∂rstd/∂var = −rstd / 2(var + ε); the one-pass variance cancels against mean z²).
GEMMs   |err| <= (ε_p + R·u + ε_s)·S, S the same product with absolute values in fp64, R the
        reduction length. ε_p = 2^-16 is the per-product constant of hi·hi + hi·lo + lo·hi against a·b
        that this scheme was specified with (|lo| <= 2^-9|x|, lo rounded once more, lo·lo dropped:
        3·2^-18). That derivation holds for the typical element only: bf16 keeps 8 significant bits,
        so the guaranteed |lo| is 2^-8|x| and a single product can miss by 3·2^-16; S has to be
        carried by one product whose two factors both round worst for that. The asserted constant
        stays 2^-16 (nothing here is fitted to the kernels); the worst observed error / bound is 0.90,
        at N = 8, where S has the fewest terms. R·u charges every fp32 product one
        rounding of the running sum. ε_s, the fp32 roundings outside the MFMA chain: a standardised
        element is fl(fl(z − μ)·rstd) = ẑ*(1 + 2u) against ẑ* = (z − μ)·rstd of the SAME fp32 μ, rstd, so
        it does not grow with |μ|/σ; C has two standardised operands (4u), the division by N (u) and
        the second-order terms (u): ε_s = 6u. The backward GEMM has one standardised operand: ε_s = 4u.
G, r    G is one or two roundings of the kernel's C: 2u|G|. A term G·C carries 2u more. r1 adds
        4·ceil(D/1024) terms per thread, 6 butterfly steps, 3 waves, then divides: n1 roundings;
        r2 adds the 8 rows of a block in fp32, the blocks in fp64, divides and rounds: 10.
loss    A term is at most 3 roundings ((C − 1)², λ·C²), a thread adds T = 32·ceil(D/1024) of them in
        fp32, everything after that is fp64, then one rounding: (T + 4)·u·L, all terms >= 0.
dz      rstd·(val − ẑ·r)·g: val carries the GEMM bound; ẑ 2u, the product, the difference and the two
        scalings one rounding each: |rstd·g|·(B_val + 4u·(|ẑ*·r| + |val − ẑ*·r|)).
"""
import pytest
import torch

import headgemm_checks as CK
from aux_oracle import f32_value

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = CK.U
EPS_P = 2.0 ** -16
EPS = 1e-5
SHAPES = [(8, 64), (40, 192), (264, 320), (64, 2048)]
WORST = CK.Worst()


def views(N, D, seed=0):
    """z2 = 0.5·z1 + noise; column scales 0.1 … 10, offsets up to 8 scales; column 3 constant."""
    gen = torch.Generator().manual_seed(seed + 31 * N + D)
    scale = 10.0 ** (2 * torch.rand(D, generator=gen, dtype=F64) - 1)
    off = scale * 8 * (2 * torch.rand(D, generator=gen, dtype=F64) - 1)
    z1 = torch.randn(N, D, generator=gen, dtype=F64) * scale + off
    z2 = 0.5 * z1 + torch.randn(N, D, generator=gen, dtype=F64) * scale
    z1[:, 3], z2[:, 3] = 2.5, -1.25
    return z1.float(), z2.float()


_CASE = {}


def case(N, D, lam, dev):
    """The kernels' stage outputs (CPU tensors), computed once per (N, D, λ)."""
    if (N, D, lam) not in _CASE:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require()
        z1, z2 = (t.to(dev) for t in views(N, D))
        stats = m.barlow_colstats(z1, z2, EPS)[1]
        C = m.barlow_xcorr(z1, z2, stats)
        C0 = C.clone()
        loss, G, r = m.barlow_loss_grad(C, lam, N)
        assert G.data_ptr() == C.data_ptr()
        g = torch.tensor([1.7], device=dev)
        dz1, dz2 = m.barlow_bwd(z1, z2, G, stats, r, g)
        torch.cuda.synchronize()
        _CASE[N, D, lam] = {k: v.cpu() for k, v in dict(z1=z1, z2=z2, stats=stats, C=C0, loss=loss, G=G, r=r,
                                                        dz1=dz1, dz2=dz2).items()}
    return _CASE[N, D, lam]


def zhat(c):
    """ẑ* of both views in fp64 from the kernel's fp32 stats."""
    st = c["stats"].to(F64)
    return (c["z1"].to(F64) - st[0, 0]) * st[0, 1], (c["z2"].to(F64) - st[1, 0]) * st[1, 1]


@pytest.mark.parametrize("N,D", SHAPES)
def test_stats_and_xcorr(gpu, N, D):
    c = case(N, D, 0.0051, gpu)
    ctx = f"[N={N} D={D}]"
    for v, z in enumerate((c["z1"].to(F64), c["z2"].to(F64))):
        mu, msq = z.mean(0), (z * z).mean(0)
        var = ((z - mu) ** 2).mean(0)
        rstd = (var + EPS).rsqrt()
        e64 = (N + 4) * 2.0 ** -52
        CK.within(WORST, "mu", c["stats"][v, 0], mu, U * mu.abs() + e64 * z.abs().mean(0), ctx)
        CK.within(WORST, "rstd", c["stats"][v, 1], rstd, rstd * (U + e64 * msq / (var + EPS)), ctx)
    assert torch.equal(c["stats"][:, 0, 3], torch.tensor([2.5, -1.25]))
    h1, h2 = zhat(c)
    assert not h1[:, 3].any() and not h2[:, 3].any()
    S = h1.abs().t() @ h2.abs() / N
    CK.within(WORST, "C", c["C"], h1.t() @ h2 / N, (EPS_P + N * U + 6 * U) * S, ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("lam", [0.0051, 1.0])
@pytest.mark.parametrize("N,D", SHAPES)
def test_loss_grad_and_backward(gpu, N, D, lam):
    c = case(N, D, lam, gpu)
    ctx = f"[N={N} D={D} lam={lam}]"
    l32 = f32_value(lam)
    C = c["C"].to(F64)
    eye = torch.eye(D, dtype=torch.bool)
    G = torch.where(eye, 2 * (C - 1), 2 * l32 * C)
    T = torch.where(eye, (C - 1) ** 2, l32 * C * C)
    GC = G * C
    k = -(-D // 1024)
    CK.within(WORST, "G", c["G"], G, 2 * U * G.abs(), ctx)
    CK.within(WORST, "r1", c["r"][0], GC.sum(1) / N, 1.01 * (2 + 4 * k + 10) * U * GC.abs().sum(1) / N, ctx)
    CK.within(WORST, "r2", c["r"][1], GC.sum(0) / N, 1.01 * (2 + 10) * U * GC.abs().sum(0) / N, ctx)
    CK.within(WORST, "loss", c["loss"].reshape(1), T.sum().reshape(1), 1.01 * (32 * k + 4) * U * T.sum(), ctx)
    # backward on the kernel's own G, r and stats
    h1, h2 = zhat(c)
    Gk, r, st, g = c["G"].to(F64), c["r"].to(F64), c["stats"].to(F64), f32_value(1.7)
    for name, ho, hv, B, v in (("dz1", h2, h1, Gk.t(), 0), ("dz2", h1, h2, Gk, 1)):
        val = ho @ B / N
        B_val = (EPS_P + D * U + 4 * U) * (ho.abs() @ B.abs() / N)
        inner = val - hv * r[v]
        bound = (st[v, 1] * g).abs() * (B_val + 4 * U * ((hv * r[v]).abs() + inner.abs()))
        CK.within(WORST, name, c[name], st[v, 1] * inner * g, bound, ctx)
    print(ctx, WORST.report())


def _definition(z1, z2, lam):
    """The plain definition in the dtype of its inputs (fp64 here), for autograd."""
    h1 = (z1 - z1.mean(0)) / (z1.var(0, unbiased=False) + EPS).sqrt()
    h2 = (z2 - z2.mean(0)) / (z2.var(0, unbiased=False) + EPS).sqrt()
    C = h1.t() @ h2 / z1.shape[0]
    eye = torch.eye(C.shape[0], dtype=C.dtype)
    return (((C - 1) ** 2) * eye).sum() + lam * ((C * C) * (1 - eye)).sum()


def test_module_end_to_end(gpu):
    """BarlowTwinsLoss (native) against fp64 autograd of the definition: catches swapped views, a
    transposed G, a wrong N. Tolerances relative to the largest entry: three chained stages, each
    within about 2^-15 of its absolute-value product (R·u <= 2^-16 here, ε_p = 2^-16), and that
    product up to 2^3 times the entry at these shapes: 3·2^-12 < 1e-3; the loss is one sum of D²
    non-negative terms of C: 1e-4."""
    from simclr_pytorch_distributed_amd.losses import BarlowTwinsLoss
    N, D, lam = 40, 192, 0.0051
    z1, z2 = views(N, D, seed=7)
    feats = torch.cat([z1, z2]).to(gpu).requires_grad_(True)
    loss = BarlowTwinsLoss(lam, backend="native")(feats)
    (1.7 * loss).backward()
    a, b = z1.to(F64).requires_grad_(True), z2.to(F64).requires_grad_(True)
    ref = _definition(a, b, lam)
    (1.7 * ref).backward()
    gref = torch.cat([a.grad, b.grad])
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    err = (feats.grad.cpu().to(F64) - gref).abs().max().item()
    print(f"e2e loss {loss.item():.6f} ref {ref.item():.6f} grad err/max {err / gref.abs().max().item():.3g}")
    assert err <= 1e-3 * gref.abs().max().item()


def test_bit_identical_runs(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    z1, z2 = (t.to(gpu) for t in views(264, 320))
    g = torch.ones(1, device=gpu)
    outs = []
    for _ in range(2):
        loss, G, stats, r = m.barlow_fwd(z1, z2, 0.0051, EPS)
        outs.append([loss, G, stats, r, *m.barlow_bwd(z1, z2, G, stats, r, g)])
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_engine_step(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.ops import barlow
    calls = []
    native = barlow.barlow_loss
    monkeypatch.setattr(barlow, "barlow_loss", lambda *a: calls.append(1) or native(*a))
    opt = parse_pretrain(["--method", "BarlowTwins", "--model", "resnet18", "--synthetic", "--synthetic_size", "64",
                          "--batch_size", "32", "--feat_dim", "128", "--max_steps", "2", "--backend", "native",
                          "--work_dir", str(tmp_path)], make_dirs=False)
    eng = PretrainEngine(opt)
    w0 = eng.flat.flat.clone()
    for it in range(opt.max_steps):
        st = eng.train_step(torch.arange(32 * it, 32 * it + 32, device=gpu), 1, it, 2)
        assert torch.isfinite(st["loss_local"]).item()
    assert len(calls) == 2 and not torch.equal(w0, eng.flat.flat) and torch.isfinite(eng.flat.flat).all().item()
