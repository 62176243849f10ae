"""Barlow Twins loss on the CPU: the torch twin against the definition written out independently,
the analytic backward that csrc/kernels/barlow.hip implements, the flags, and two gloo ranks
against one process."""
import pytest
import torch
import torch.distributed as dist

from test_dist import _run

F64 = torch.float64
EPS = 1e-5
SHAPES = [(8, 64), (40, 192), (264, 320)]


def _views(N, D):
    gen = torch.Generator().manual_seed(N + D)
    z1 = torch.randn(N, D, generator=gen, dtype=F64) * 3 + torch.randn(D, generator=gen, dtype=F64) * 5
    return z1, 0.5 * z1 + torch.randn(N, D, generator=gen, dtype=F64)


def _definition(z1, z2, lam):
    N, D = z1.shape
    h1 = (z1 - z1.mean(0)) / (z1.var(0, unbiased=False) + EPS).sqrt()
    h2 = (z2 - z2.mean(0)) / (z2.var(0, unbiased=False) + EPS).sqrt()
    C = h1.t() @ h2 / N
    eye = torch.eye(D, dtype=F64)
    return (((C - 1) ** 2) * eye).sum() + lam * ((C * C) * (1 - eye)).sum()


@pytest.mark.parametrize("lam", [0.0051, 1.0])
@pytest.mark.parametrize("N,D", SHAPES)
def test_reference_and_analytic_backward(N, D, lam):
    from simclr_pytorch_distributed_amd.losses import barlow_reference
    z1, z2 = _views(N, D)
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    ref = _definition(a, b, lam)
    (1.7 * ref).backward()
    p, q = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    twin = barlow_reference(p, q, lam, EPS)
    (1.7 * twin).backward()
    assert abs(twin.item() - ref.item()) <= 1e-12 * abs(ref.item())
    scale = max(a.grad.abs().max().item(), b.grad.abs().max().item())
    assert (p.grad - a.grad).abs().max().item() <= 1e-12 * scale
    assert (q.grad - b.grad).abs().max().item() <= 1e-12 * scale
    # the kernels' backward: dz_v = rstd_v ⊙ (ẑ_o·G^(ᵀ)/N − ẑ_v ⊙ r_v)·g, r from C and G alone
    rs1, rs2 = (z1.var(0, unbiased=False) + EPS).rsqrt(), (z2.var(0, unbiased=False) + EPS).rsqrt()
    h1, h2 = (z1 - z1.mean(0)) * rs1, (z2 - z2.mean(0)) * rs2
    C = h1.t() @ h2 / N
    eye = torch.eye(D, dtype=torch.bool)
    G = torch.where(eye, 2 * (C - 1), 2 * lam * C)
    r1, r2 = (G * C).sum(1) / N, (G * C).sum(0) / N
    dz1 = rs1 * (h2 @ G.t() / N - h1 * r1) * 1.7
    dz2 = rs2 * (h1 @ G / N - h2 * r2) * 1.7
    assert (dz1 - a.grad).abs().max().item() <= 1e-12 * scale
    assert (dz2 - b.grad).abs().max().item() <= 1e-12 * scale


def test_flags(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    base = ["--synthetic", "--work_dir", str(tmp_path)]
    opt = parse_pretrain(base + ["--method", "BarlowTwins", "--bt_lambda", "0.01"], make_dirs=False)
    assert opt.method == "BarlowTwins" and opt.bt_lambda == 0.01
    assert "bt_lambda" not in vars(parse_pretrain(base + ["--method", "BarlowTwins"], make_dirs=False))
    assert "bt_lambda" not in vars(parse_pretrain(base + ["--method", "SimCLR"], make_dirs=False))
    with pytest.raises(ValueError):
        parse_pretrain(base + ["--bt_lambda", "0.01"], make_dirs=False)


def _two_rank_case(rank, world, d):
    from simclr_pytorch_distributed_amd.losses import BarlowTwinsLoss, barlow_reference
    z1, z2 = _views(12 * world, 64)
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    ref = _definition(a, b, 0.0051)
    ref.backward()
    n = 12
    sl = slice(rank * n, (rank + 1) * n)
    loc = torch.cat([z1[sl], z2[sl]]).clone().requires_grad_(True)
    loss = BarlowTwinsLoss(0.0051, backend="torch")(loc)
    loss.backward()
    tot = loss.detach().clone()
    dist.all_reduce(tot)
    assert abs(tot.item() - ref.item()) <= 1e-12 * abs(ref.item())
    gref = torch.cat([a.grad[sl], b.grad[sl]])
    assert (loc.grad - gref).abs().max().item() <= 1e-12 * gref.abs().max().item()
    assert barlow_reference(z1[sl], z2[sl]).item() == pytest.approx(ref.item(), rel=1e-12)


def test_two_ranks_equal_one_process():
    _run(_two_rank_case, 2)
