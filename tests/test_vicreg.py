"""VICReg loss on the CPU: the torch twin against the definition written out independently, the
analytic backward that csrc/kernels/vicreg.hip implements, the flags, and two gloo ranks against
one process."""
import pytest
import torch
import torch.distributed as dist

from test_dist import _run

F64 = torch.float64
EPS = 1e-4
SHAPES = [(8, 64), (40, 192), (264, 320)]
WEIGHTS = [(25.0, 25.0, 1.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0)]


def _views(N, D):
    """Column scales 0.1 … 10: the hinge is active in some columns and not in others."""
    gen = torch.Generator().manual_seed(N + D)
    scale = 10.0 ** (2 * torch.rand(D, generator=gen, dtype=F64) - 1)
    z1 = torch.randn(N, D, generator=gen, dtype=F64) * scale + torch.randn(D, generator=gen, dtype=F64) * 5
    return z1, 0.5 * z1 + torch.randn(N, D, generator=gen, dtype=F64) * scale


def _definition(z1, z2, sim, std, cov):
    """The official formulation: mse_loss, relu(1 − sqrt(var + ε)), off-diagonal of the covariance."""
    N, D = z1.shape
    loss = sim * torch.nn.functional.mse_loss(z1, z2)
    for z in (z1, z2):
        x = z - z.mean(0)
        c = x.t() @ x / (N - 1)
        off = c - torch.diag(torch.diagonal(c))
        loss = loss + std * torch.relu(1 - (z.var(0) + EPS).sqrt()).mean() / 2 + cov * off.pow(2).sum() / D
    return loss


@pytest.mark.parametrize("sim,std,cov", WEIGHTS)
@pytest.mark.parametrize("N,D", SHAPES)
def test_reference_and_analytic_backward(N, D, sim, std, cov):
    from simclr_pytorch_distributed_amd.losses import vicreg_reference
    z1, z2 = _views(N, D)
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    ref = _definition(a, b, sim, std, cov)
    (1.7 * ref).backward()
    p, q = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    twin = vicreg_reference(p, q, sim, std, cov, EPS)
    (1.7 * twin).backward()
    assert abs(twin.item() - ref.item()) <= 1e-12 * abs(ref.item())
    scale = max(a.grad.abs().max().item(), b.grad.abs().max().item())
    assert (p.grad - a.grad).abs().max().item() <= 1e-12 * scale
    assert (q.grad - b.grad).abs().max().item() <= 1e-12 * scale
    # the kernels' backward: dz_v = g·(x̄_v·G_v − coef_v ⊙ x̄_v + 2λ/(N·D)·(z_v − z_other)); no term for
    # the centring, every column of x̄ sums to zero
    for z, zo, want in ((z1, z2, a.grad), (z2, z1, b.grad)):
        x = z - z.mean(0)
        C = x.t() @ x / (N - 1)
        S = (torch.diagonal(C) + EPS).sqrt()
        assert (S < 1).any() and (S > 1).any()
        G = 4 * cov / (D * (N - 1)) * (C - torch.diag(torch.diagonal(C)))
        coef = std * (S < 1) / (2 * D * (N - 1) * S)
        dz = 1.7 * (x @ G - coef * x + 2 * sim / (N * D) * (z - zo))
        assert (dz - want).abs().max().item() <= 1e-12 * scale


def test_flags(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    base = ["--synthetic", "--work_dir", str(tmp_path)]
    opt = parse_pretrain(base + ["--method", "VICReg", "--vic_sim", "10", "--vic_cov", "0.5"], make_dirs=False)
    assert opt.method == "VICReg" and opt.vic_sim == 10 and opt.vic_cov == 0.5 and "vic_std" not in vars(opt)
    for method in ("VICReg", "SimCLR"):
        assert not [k for k in vars(parse_pretrain(base + ["--method", method], make_dirs=False)) if k.startswith("vic_")]
    for flag in ("--vic_sim", "--vic_std", "--vic_cov"):
        with pytest.raises(ValueError):
            parse_pretrain(base + [flag, "1"], make_dirs=False)
        for bad in ("-1", "inf", "nan"):
            with pytest.raises(ValueError):
                parse_pretrain(base + ["--method", "VICReg", flag, bad], make_dirs=False)


def _two_rank_case(rank, world, d):
    from simclr_pytorch_distributed_amd.losses import VICRegLoss, vicreg_reference
    z1, z2 = _views(12 * world, 64)
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    ref = _definition(a, b, 25.0, 25.0, 1.0)
    ref.backward()
    n = 12
    sl = slice(rank * n, (rank + 1) * n)
    loc = torch.cat([z1[sl], z2[sl]]).clone().requires_grad_(True)
    loss = VICRegLoss(backend="torch")(loc)
    loss.backward()
    tot = loss.detach().clone()
    dist.all_reduce(tot)
    assert abs(tot.item() - ref.item()) <= 1e-12 * abs(ref.item())
    gref = torch.cat([a.grad[sl], b.grad[sl]])
    assert (loc.grad - gref).abs().max().item() <= 1e-12 * gref.abs().max().item()
    assert vicreg_reference(z1[sl], z2[sl]).item() == pytest.approx(ref.item(), rel=1e-12)


def test_two_ranks_equal_one_process():
    _run(_two_rank_case, 2)
