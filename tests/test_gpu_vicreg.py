"""The VICReg kernels (csrc/kernels/vicreg.hip) on the GPU, stage by stage against fp64, so that no
bound is composed through the chain: every stage's reference is evaluated in fp64 on the kernel's
OWN inputs to that stage (its fp32 mu, its sums, its C, its G and coef).

u = 2^-24 (headgemm_checks.U). The bounds are derived here, none is measured (worst error / bound
per stage on an MI355X: profiles/vicreg.txt).

sums    fp64 throughout: (N + 4)·2^-52 of Σ|z| resp. Σ(z1 − z2)² (z1 − z2 is exact in fp64).
mu      one rounding of the fp64 mean: |Δμ| <= u·|μ| + (N + 4)·2^-52·mean|z|.
GEMMs   |err| <= (ε_p + R·u + ε_s)·S, S the same product with absolute values in fp64, R the reduction
        length. ε_p = 2^-16 is the per-product constant of hi·hi + hi·lo + lo·hi against a·b that this
        scheme is specified with (typical element; see tests/test_gpu_barlow.py for the worst one).
        R·u charges every fp32 product one rounding of the running sum. ε_s, the fp32 roundings
        outside the MFMA chain: a centred element is fl(z − μ) = x*(1 + u) against x* = z − μ of the
        SAME fp32 μ. C has two centred operands (2u), the division by N − 1 (u, N − 1 exact in fp32)
        and the second-order terms (u): ε_s = 4u. The backward GEMM has one centred operand: ε_s = 2u.
G       one rounding of scale·C with scale = fp32(4ν/(D(N − 1))): 2u|G|; the diagonal is exactly 0.
coef    S = sqrt(fl(C_jj + ε)) correctly rounded: (u/2 + u)·S; cf / S one more rounding: 4u·|coef|. The
        indicator [S < 1] agrees with fp64 because the inputs keep |S − 1| > 2^-20 (asserted first).
terms   L_sim: an fp64 sum of the kernel's third sums row, one rounding: 2u. L_std: a hinge term
        relu(1 − S) is off by at most 2u·S + u <= 3u, a thread adds at most 4 of them in fp32 (3u of
        their sum), the rest is fp64: (3u·#active + 4u·Σh)/(2D) + u·L_std. L_cov: a term C² is one
        rounding, a thread adds T = 32·ceil(D/1024) of them in fp32, then fp64 and one rounding:
        1.01·(T + 4)·u·L_cov, all terms >= 0. loss: the weighted fp64 sum, rounded once.
dz      g·(a − b + c), a = x̄·G under the GEMM bound, b = coef·fl(z − μ) (2u), c = sim2·fl(z_v − z_o)
        (2u), two additions and the scaling (u of their partial results each, <= |a| + |b| + |c|):
        |g|·(B_a + 6u·(|a| + |b| + |c|)).
"""
import pytest
import torch

import headgemm_checks as CK
from aux_oracle import f32_value

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = CK.U
EPS_P = 2.0 ** -16
EPS = 1e-4
SHAPES = [(8, 64), (40, 192), (264, 320), (64, 2048)]
WEIGHTS = [(25.0, 25.0, 1.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0)]
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


def fair_inputs(z1, z2, margin):
    """The condition on the inputs: no S of the fp64 definition within `margin` of the hinge's kink,
    and S on both sides of it."""
    S = torch.stack([(z.to(F64).var(0) + EPS).sqrt() for z in (z1, z2)])
    assert ((S - 1).abs() > margin).all() and (S < 1).any() and (S > 1).any()


_CASE = {}


def case(N, D, w, dev):
    """The kernels' stage outputs (CPU tensors), computed once per (N, D, weights)."""
    if (N, D, w) not in _CASE:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require()
        z1, z2 = views(N, D)
        fair_inputs(z1, z2, 2.0 ** -20)
        z1, z2 = z1.to(dev), z2.to(dev)
        sums, mu = m.vicreg_colstats(z1, z2)
        C = m.vicreg_cov(z1, z2, mu)
        C0 = C.clone()
        loss, terms, G, coef = m.vicreg_loss_grad(C, sums, *w, EPS, N)
        assert G.data_ptr() == C.data_ptr()
        g = torch.tensor([1.7], device=dev)
        dz1, dz2 = m.vicreg_bwd(z1, z2, G, mu, coef, g, w[0])
        torch.cuda.synchronize()
        _CASE[N, D, w] = {k: v.cpu() for k, v in dict(z1=z1, z2=z2, sums=sums, mu=mu, C=C0, loss=loss, terms=terms,
                                                      G=G, coef=coef, dz1=dz1, dz2=dz2).items()}
    return _CASE[N, D, w]


def centred(c):
    """x* of both views in fp64 from the kernel's fp32 mu."""
    mu = c["mu"].to(F64)
    return c["z1"].to(F64) - mu[0], c["z2"].to(F64) - mu[1]


@pytest.mark.parametrize("N,D", SHAPES)
def test_stats_and_cov(gpu, N, D):
    c = case(N, D, WEIGHTS[0], gpu)
    ctx = f"[N={N} D={D}]"
    z = [c["z1"].to(F64), c["z2"].to(F64)]
    e64 = (N + 4) * 2.0 ** -52
    for v in range(2):
        CK.within(WORST, "sums", c["sums"][v], z[v].sum(0), e64 * z[v].abs().sum(0), ctx)
        CK.within(WORST, "mu", c["mu"][v], z[v].mean(0), U * z[v].mean(0).abs() + e64 * z[v].abs().mean(0), ctx)
    d2 = ((z[0] - z[1]) ** 2).sum(0)
    CK.within(WORST, "sums", c["sums"][2], d2, e64 * d2, ctx)
    assert torch.equal(c["mu"][:, 3], torch.tensor([2.5, -1.25]))
    for v, x in enumerate(centred(c)):
        Cv = c["C"][v]
        assert torch.equal(Cv, Cv.t()), f"{ctx} C[{v}] is not symmetric bit for bit"
        assert Cv[3, 3].item() == 0.0 and not Cv[3].any()
        CK.within(WORST, "C", Cv, x.t() @ x / (N - 1), (EPS_P + N * U + 4 * U) * (x.abs().t() @ x.abs() / (N - 1)), ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("N,D", SHAPES)
def test_loss_grad_and_backward(gpu, N, D, w):
    c = case(N, D, w, gpu)
    ctx = f"[N={N} D={D} w={w}]"
    sim, std, cov = w
    C = c["C"].to(F64)
    var = torch.diagonal(C, dim1=1, dim2=2)
    S = (var + f32_value(EPS)).sqrt()
    assert ((S - 1).abs() > 2.0 ** -20).all()
    eye = torch.eye(D, dtype=torch.bool)
    G = torch.where(eye, torch.zeros((), dtype=F64), f32_value(4 * cov / (D * (N - 1))) * C)
    coef = f32_value(std / (2.0 * (D * (N - 1.0)))) * (S < 1) / S
    assert not torch.diagonal(c["G"], dim1=1, dim2=2).any()
    CK.within(WORST, "G", c["G"], G, 2 * U * G.abs(), ctx)
    CK.within(WORST, "coef", c["coef"], coef, 4 * U * coef.abs(), ctx)
    hinge = torch.relu(1 - S)
    l_sim = c["sums"][2].sum() / (N * D)
    l_std = 0.5 * hinge.sum() / D
    l_cov = ((C * C).sum() - (var * var).sum()) / D
    T = 32 * -(-D // 1024)
    B = torch.stack([2 * U * l_sim, (3 * U * (S < 1).sum() + 4 * U * hinge.sum()) / (2 * D) + U * l_std,
                     1.01 * (T + 4) * U * l_cov])
    ref = torch.stack([l_sim, l_std, l_cov])
    wt = torch.tensor(w, dtype=F64)
    CK.within(WORST, "terms", c["terms"], ref, B, ctx)
    CK.within(WORST, "loss", c["loss"], (wt * ref).sum().reshape(1), (wt * B).sum() + U * (wt * ref).sum(), ctx)
    # backward on the kernel's own G, mu and coef
    x = centred(c)
    z = [c["z1"].to(F64), c["z2"].to(F64)]
    g, sim2 = f32_value(1.7), f32_value(2 * sim / (N * float(D)))
    for v, name in enumerate(("dz1", "dz2")):
        Gk = c["G"][v].to(F64)
        a = x[v] @ Gk
        b = c["coef"][v].to(F64) * x[v]
        s = sim2 * (z[v] - z[1 - v])
        B_a = (EPS_P + D * U + 2 * U) * (x[v].abs() @ Gk.abs())
        CK.within(WORST, name, c[name], g * (a - b + s), g * (B_a + 6 * U * (a.abs() + b.abs() + s.abs())), ctx)
    print(ctx, WORST.report())


def _definition(z1, z2, sim, std, cov):
    """The plain definition in the dtype of its inputs (fp64 here), for autograd."""
    N, D = z1.shape
    loss = sim * ((z1 - z2) ** 2).sum() / (N * D)
    for z in (z1, z2):
        C = torch.cov(z.t())
        loss = loss + std * torch.relu(1 - (torch.diagonal(C) + EPS).sqrt()).mean() / 2
        loss = loss + cov * ((C * C).sum() - (torch.diagonal(C) ** 2).sum()) / D
    return loss


def test_module_end_to_end(gpu):
    """VICRegLoss (native) against fp64 autograd of the definition: catches swapped views, a wrong
    sign on the invariance term, N for N − 1. Tolerances relative to the largest entry, as for Barlow
    Twins: the gradient passes two chained GEMM stages (C, then x̄·G), each within about 2^-15 of
    its absolute-value product (R·u <= 2^-16 here, ε_p = 2^-16), and that product up to 2^3 times the
    entry at these shapes: 2·2^-12 < 1e-3; the loss is sums of non-negative terms of C, S and
    (z1 − z2)²: 1e-4."""
    from simclr_pytorch_distributed_amd.losses import VICRegLoss
    N, D, w = 40, 192, WEIGHTS[0]
    z1, z2 = views(N, D, seed=7)
    fair_inputs(z1, z2, 1e-3)
    feats = torch.cat([z1, z2]).to(gpu).requires_grad_(True)
    loss = VICRegLoss(*w, backend="native")(feats)
    (1.7 * loss).backward()
    a, b = z1.to(F64).requires_grad_(True), z2.to(F64).requires_grad_(True)
    ref = _definition(a, b, *w)
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
        loss, terms, G, mu, coef = m.vicreg_fwd(z1, z2, 25.0, 25.0, 1.0, EPS)
        outs.append([loss, terms, G, mu, coef, *m.vicreg_bwd(z1, z2, G, mu, coef, g, 25.0)])
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_engine_step(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.ops import vicreg
    calls = []
    native = vicreg.vicreg_loss
    monkeypatch.setattr(vicreg, "vicreg_loss", lambda *a: calls.append(1) or native(*a))
    opt = parse_pretrain(["--method", "VICReg", "--model", "resnet18", "--synthetic", "--synthetic_size", "64",
                          "--batch_size", "32", "--feat_dim", "128", "--max_steps", "2", "--backend", "native",
                          "--work_dir", str(tmp_path)], make_dirs=False)
    eng = PretrainEngine(opt)
    w0 = eng.flat.flat.clone()
    for it in range(opt.max_steps):
        st = eng.train_step(torch.arange(32 * it, 32 * it + 32, device=gpu), 1, it, 2)
        assert torch.isfinite(st["loss_local"]).item()
    assert len(calls) == 2 and not torch.equal(w0, eng.flat.flat) and torch.isfinite(eng.flat.flat).all().item()
