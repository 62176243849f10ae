"""The BatchNorm projector kernels (csrc/kernels/head_bn.hip) on the GPU, stage by stage against fp64
on each stage's OWN inputs (the kernel's yb for everything after the GEMM; its μ, rstd for the
activation and the backward), so that no bound is composed through the chain.

u = 2^-24 (one fp32 rounding), b = 2^-8 (one bf16 rounding: 8 significant bits). Every bound is derived from the
kernel's arithmetic, none is measured; worst error / bound per stage on an MI355X: profiles/head_bn.txt.

yb      bf16 of an fp32 MFMA sum of K exact products: |yb − y*| <= b·|y*| + (1 + b)·K·u·S, S = |x|·|w|ᵀ.
sums    a column sum runs in-lane over <= 16 fragments (forward) / <= 8 rows (backward), then 4 DPP
        levels, then <= 16 partials: at most A = 32 additions on any path, each one rounding of a
        partial sum: A·u·Σ|term|.
μ       sum bound, one division: (A + 1)·u·mean|yb|. A constant column c sums exactly (k·c has
        <= 8 + 11 bits) and divides exactly: μ = c, every yb − μ = 0, rstd = 1/sqrt(ε) to one rounding.
σ²      d = fl(yb − μ) (u), d·d (u), the sum (A·u), /N (u), and the fp64 variance about the kernel's
        μ exceeds the true one by (Δμ)²: (A + 4)·u·σ² + B_μ².
rstd    1/sqrt(σ² + ε): half the relative error of σ² + ε, sqrt, division, the fp32 ε and the
        addition (4u): rstd·(B_σ²/(2(σ² + ε)) + 4u).
running (1 − m)·r + m·s: the two products, the factor 1 − m (and N/(N − 1) of the variance), the
        sum: 4u·((1 − m)|r| + m|s|) + m·(bound of s).
a       x̂ = fl(fl(yb − μ)·rstd) (2u), v = fma(γ, x̂, β) (u): B_v = 3u·(|γx̂| + |β|); ReLU is
        1-Lipschitz, then bf16: b·relu(v*) + (1 + b)·B_v.
mask    [v > 0] differs from fp64 only where |v*| <= B_v. Elements with |v*| <= 8u·(|γx̂| + |β|) are
        ambiguous: at most 0.1 % (asserted; 0 for these inputs in fp64 on the CPU), left out of the
        dy comparison, and their |da| (·|x̂|) is added to the bounds of the two sums.
dβ, dγ  A·u·Σ|dŷ| resp. (A + 3)·u·Σ|dŷ·x̂| (x̂ 2u, the product u), the sink addition u·(|sink| + |sum|).
dy      γ·rstd·(dŷ − dβ/N − x̂·dγ/N): the sums' bounds over N, 8u of (|dŷ| + |dβ/N| + |x̂·dγ/N|) for
        1/N, x̂, the products, the subtractions and the scale, then bf16: b·|dy*| + (1 + b)·E.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
U, B16, A_ADD = 2.0 ** -24, 2.0 ** -8, 32
EPS, MOM = 1e-5, 0.1
# (N, K, H): one partial fragment / one chunk; padding rows, odd chunk count, 6 or 3 strips;
# rows across every wave with a ragged tail; the maximum-rows register configuration
SHAPES = [(8, 64, 32), (24, 192, 96), (264, 128, 64), (2048, 64, 32)]
CASES = [(s, w) for s in SHAPES for w in (16, 32) if not (w == 32 and s[0] > 1024)]
WORST = {}


def within(name, got, ref, bound):
    got, ref = got.to(F64), ref.to(F64)
    assert not torch.isnan(got).any(), name
    r = float(((got - ref).abs() / (bound + 1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"head_bn worst {name} {r:.3f}")
    assert r <= 1.0, f"{name}: error / bound {r:.3f}"


def inputs(N, K, H):
    """bf16 x, w; x[:, 0] = 1 carries a per-column offset (non-zero means); output column scales
    0.1 … 10; output column 3 is the constant 2.5."""
    gen = torch.Generator().manual_seed(7 * N + K + H)
    x = torch.randn(N, K, generator=gen)
    x[:, 0] = 1.0
    scale = 10.0 ** (2 * torch.rand(H, 1, generator=gen) - 1)
    w = torch.randn(H, K, generator=gen) * scale / K ** 0.5
    w[:, 0] = (scale * 4 * (2 * torch.rand(H, 1, generator=gen) - 1))[:, 0]
    w[3] = 0.0
    w[3, 0] = 2.5
    gamma = 0.5 + torch.rand(H, generator=gen)
    beta = 0.5 * torch.randn(H, generator=gen)
    da = torch.randn(N, H, generator=gen).bfloat16()
    return x.bfloat16(), w.bfloat16(), gamma, beta, da


_CASE = {}


def case(shape, strip, dev):
    """The kernels' stage outputs (CPU tensors), computed once per case."""
    if (shape, strip) not in _CASE:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require()
        x, w, gamma, beta, da = (t.to(dev) for t in inputs(*shape))
        H = shape[2]
        rm0, rv0 = torch.linspace(-1, 1, H, device=dev), torch.linspace(0.5, 2, H, device=dev)
        sg0, sb0 = torch.linspace(-2, 2, H, device=dev), torch.linspace(3, -3, H, device=dev)
        out = []
        for _ in range(2):      # twice on the same inputs: bit-identical
            rm, rv, sg, sb = rm0.clone(), rv0.clone(), sg0.clone(), sb0.clone()
            a, yb, mu, rstd = m.head_bn_layer_fwd(x, w, gamma, beta, rm, rv, MOM, EPS, strip)
            dy = m.head_bn_layer_bwd(da, yb, mu, rstd, gamma, beta, sg, sb)
            out.append(dict(a=a, yb=yb, mu=mu, rstd=rstd, rm=rm, rv=rv, sg=sg, sb=sb, dy=dy))
        torch.cuda.synchronize()
        for k in out[0]:
            assert torch.equal(out[0][k], out[1][k]), f"{k} differs between two calls"
        c = {k: v.cpu() for k, v in out[0].items()}
        c.update(x=x.cpu(), w=w.cpu(), gamma=gamma.cpu(), beta=beta.cpu(), da=da.cpu(), rm0=rm0.cpu(), rv0=rv0.cpu(),
                 sg0=sg0.cpu(), sb0=sb0.cpu())
        _CASE[shape, strip] = c
    return _CASE[shape, strip]


@pytest.mark.parametrize("shape,strip", CASES)
def test_forward_stages(gpu, shape, strip):
    c = case(shape, strip, gpu)
    N, K, H = shape
    x, w = c["x"].to(F64), c["w"].to(F64)
    y_ref, S = x @ w.t(), x.abs() @ w.abs().t()
    within("yb", c["yb"], y_ref, B16 * y_ref.abs() + (1 + B16) * K * U * S)
    # everything below: fp64 on the kernel's yb (the N real rows only: padding rows never count)
    y = c["yb"].to(F64)
    mu_ref, var_ref = y.mean(0), y.var(0, unbiased=False)
    B_mu = (A_ADD + 1) * U * y.abs().mean(0)
    within("mu", c["mu"], mu_ref, B_mu)
    B_var = (A_ADD + 4) * U * var_ref + B_mu ** 2
    rstd_ref = (var_ref + EPS).rsqrt()
    within("rstd", c["rstd"], rstd_ref, rstd_ref * (B_var / (2 * (var_ref + EPS)) + 4 * U))
    assert float(c["mu"][3]) == 2.5 and abs(float(c["rstd"][3]) - EPS ** -0.5) <= 4 * U * EPS ** -0.5
    rm0, rv0 = c["rm0"].to(F64), c["rv0"].to(F64)
    var_u = var_ref * N / (N - 1)
    within("running_mean", c["rm"], (1 - MOM) * rm0 + MOM * mu_ref,
           4 * U * ((1 - MOM) * rm0.abs() + MOM * mu_ref.abs()) + MOM * B_mu)
    within("running_var", c["rv"], (1 - MOM) * rv0 + MOM * var_u,
           4 * U * ((1 - MOM) * rv0 + MOM * var_u) + MOM * B_var * N / (N - 1))
    mu, rstd, g, b = (c[k].to(F64) for k in ("mu", "rstd", "gamma", "beta"))
    gx = g * (y - mu) * rstd
    v = gx + b
    B_v = 3 * U * (gx.abs() + b.abs())
    within("a", c["a"], v.clamp_min(0), B16 * v.clamp_min(0) + (1 + B16) * B_v)


@pytest.mark.parametrize("shape,strip", CASES)
def test_backward_stages(gpu, shape, strip):
    c = case(shape, strip, gpu)
    N = shape[0]
    y, mu, rstd, g, b, da = (c[k].to(F64) for k in ("yb", "mu", "rstd", "gamma", "beta", "da"))
    xh = (y - mu) * rstd
    v = g * xh + b
    amb = v.abs() <= 8 * U * ((g * xh).abs() + b.abs())
    assert float(amb.double().mean()) <= 1e-3
    dh = da * (v > 0)
    slack_b, slack_g = (da.abs() * amb).sum(0), ((da * xh).abs() * amb).sum(0)
    db, dg = dh.sum(0), (dh * xh).sum(0)
    sb0, sg0 = c["sb0"].to(F64), c["sg0"].to(F64)
    B_db = A_ADD * U * dh.abs().sum(0) + slack_b
    B_dg = (A_ADD + 3) * U * (dh * xh).abs().sum(0) + slack_g
    within("dbeta", c["sb"], sb0 + db, B_db + U * (sb0.abs() + db.abs() + (sb0 + db).abs()))
    within("dgamma", c["sg"], sg0 + dg, B_dg + U * (sg0.abs() + dg.abs() + (sg0 + dg).abs()))
    dy_ref = g * rstd * (dh - db / N - xh * dg / N)
    E = (g * rstd).abs() * (B_db / N + xh.abs() * B_dg / N + 8 * U * (dh.abs() + db.abs() / N + (xh * dg).abs() / N))
    ok = ~amb
    within("dy", c["dy"][ok], dy_ref[ok], (B16 * dy_ref.abs() + (1 + B16) * E)[ok])


def test_whole_node(gpu):
    """projection_head of a 3-layer head at (40, 128, 64), feat_dim 32, and the gradients of every
    weight, γ, β and the input, against an fp64 twin. Tolerance: torch's autocast-bf16 head has the
    same operand roundings at other points; the native error may be at most twice its error against
    the same twin, in the same (relative Frobenius) norm."""
    from simclr_pytorch_distributed_amd.models.resnet import bn_projector
    from simclr_pytorch_distributed_amd.ops.head import projection_head
    from simclr_pytorch_distributed_amd.ops.weights import ConvWeightCache
    torch.manual_seed(5)
    nat = bn_projector(128, 64, 32, 3).to(gpu)
    with torch.no_grad():
        for bn in (nat[1], nat[4]):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0, 0.5)
    twin, auto = copy.deepcopy(nat).double(), copy.deepcopy(nat)
    wc = ConvWeightCache([m for m in nat if isinstance(m, torch.nn.Linear)], None)
    wc.refresh()
    feat = torch.randn(40, 128, device=gpu)
    gz = torch.randn(40, 32, device=gpu)
    f_n, f_a, f_t = (feat.clone().to(d).requires_grad_(True) for d in (torch.float32, torch.float32, F64))
    z_n = projection_head(f_n, nat, wc)
    z_t = twin(f_t)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z_a = auto(f_a).float()
    assert z_n.dtype == torch.float32
    for z, g in ((z_n, gz), (z_a, gz), (z_t, gz.double())):
        z.backward(g)
    rel = lambda u, v: float((u.double() - v).norm() / v.norm())  # noqa: E731
    pairs = [("z", z_n, z_a, z_t), ("dfeat", f_n.grad, f_a.grad, f_t.grad)]
    pairs += [(k, p.grad, dict(auto.named_parameters())[k].grad, dict(twin.named_parameters())[k].grad)
              for k, p in nat.named_parameters()]
    for name, n, a, t in pairs:
        e_n, e_a = rel(n.detach(), t.detach()), rel(a.detach(), t.detach())
        print(f"head_bn node {name}: native {e_n:.3e} autocast {e_a:.3e}")
        assert e_n <= 2 * e_a, f"{name}: native {e_n:.3e} > 2 x autocast {e_a:.3e}"
    for bn_n, bn_t in ((nat[1], twin[1]), (nat[4], twin[4])):   # the kernel moved the running statistics
        assert rel(bn_n.running_mean, bn_t.running_mean) < 3e-2 and rel(bn_n.running_var, bn_t.running_var) < 3e-2
