"""The DINO kernels (csrc/kernels/dino.hip) on the GPU against the fp64 twin evaluated on the fp32 inputs.

End to end the tolerances are test_gpu_vicreg.py's and test_gpu_moco.py's: 1e-4 of the loss, 1e-3 of the
largest element of dz and of dV. The new centre is one fp64 dot per prototype rounded once, held to
4u·Σ_d|Ĉ_t,k,d·z̄_d| + u·|c| (u = 2^-24) against the fp64 column mean of the teacher logits.

Shapes (N per view, D, K): one row block of 8 valid rows and one prototype span; ragged spans (10 tiles in
spans of 4, 4, 2) and a sample axis cut in two; the largest D (16-row tiles, the 16x16x16 second product),
two row blocks per view and 8 sample spans; several prototype spans and dV from the sweep's epilogue.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -24
SHAPES = [(8, 64, 64), (40, 128, 320), (72, 256, 1024), (136, 128, 4096)]
TEMPS = [(0.1, 0.04), (0.1, 0.07)]
G = 1.7
M_C = 0.9


def inputs(N, D, K, seed=0):
    """Row norms spread over two decades, the teacher correlated with the student, V rows of unequal
    norms, a random non-zero centre."""
    gen = torch.Generator().manual_seed(seed + 31 * N + D + K)
    spread = lambda r: 10.0 ** (2 * torch.rand(r, 1, generator=gen, dtype=F64) - 1)
    zs = torch.randn(2 * N, D, generator=gen, dtype=F64) * spread(2 * N)
    zt = (torch.randn(2 * N, D, generator=gen, dtype=F64) + 0.7 * F.normalize(zs, dim=1) * D ** 0.5) * spread(2 * N)
    vs = torch.randn(K, D, generator=gen, dtype=F64) * spread(K)
    vs[: min(K, 2 * N)] += 2.0 * zs[: min(K, 2 * N)]      # some confident rows
    vt = vs + 0.05 * torch.randn(K, D, generator=gen, dtype=F64) * vs.norm(dim=1, keepdim=True) / D ** 0.5
    center = 0.1 * torch.randn(K, generator=gen, dtype=F64)
    return [t.float() for t in (zs, zt, vs, vt, center)]


_CASE = {}


def case(N, D, K, temps, dev):
    """Two native runs and the fp64 reference, computed once per shape and temperature pair."""
    key = (N, D, K, temps)
    if key not in _CASE:
        from simclr_pytorch_distributed_amd.losses.dino import dino_reference
        from simclr_pytorch_distributed_amd.ops import dino
        cpu = inputs(N, D, K)
        runs = []
        for _ in range(2):
            zs, zt, vs, vt, center = (t.to(dev) for t in cpu)
            zs.requires_grad_(True)
            vs.requires_grad_(True)
            loss, zsum = dino.dino_loss(zs, zt, vs, vt, center, *temps)
            (G * loss).backward()
            new_c = dino.center_update(vt, zsum, center, M_C, 2 * N)
            runs.append([t.detach().cpu() for t in (loss.reshape(1), zs.grad, vs.grad, new_c)])
        zs, zt, vs, vt, center = (t.to(F64) for t in cpu)
        zs.requires_grad_(True)
        vs.requires_grad_(True)
        ref = dino_reference(zs, zt, vs, vt, center, *temps)
        (G * ref).backward()
        ct, zbar = F.normalize(vt, dim=1), F.normalize(zt, dim=1).mean(0)
        _CASE[key] = dict(runs=runs, loss=ref.detach(), dz=zs.grad, dv=vs.grad,
                          center=M_C * center + (1 - M_C) * (F.normalize(zt, dim=1) @ ct.t()).mean(0),
                          center_bound=4 * U * (ct.abs() @ zbar.abs()))
    return _CASE[key]


@pytest.mark.parametrize("temps", TEMPS)
@pytest.mark.parametrize("N,D,K", SHAPES)
def test_loss_and_gradients(gpu, N, D, K, temps):
    c = case(N, D, K, temps, gpu)
    loss, dz, dv, _ = (t.to(F64) for t in c["runs"][0])
    e_loss = abs(loss.item() - c["loss"].item()) / abs(c["loss"].item())
    e_dz = (dz - c["dz"]).abs().max().item() / c["dz"].abs().max().item()
    e_dv = (dv - c["dv"]).abs().max().item() / c["dv"].abs().max().item()
    print(f"[N={N} D={D} K={K} temps={temps}] loss {c['loss'].item():.6f} rel err {e_loss:.3g}, dz err/max {e_dz:.3g}, "
          f"dV err/max {e_dv:.3g}")
    assert e_loss <= 1e-4 and e_dz <= 1e-3 and e_dv <= 1e-3


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_center_and_determinism(gpu, N, D, K):
    c = case(N, D, K, TEMPS[0], gpu)
    new_c = c["runs"][0][3].to(F64)
    assert ((new_c - c["center"]).abs() <= c["center_bound"] + U * c["center"].abs()).all()
    for a, b in zip(*c["runs"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    from simclr_pytorch_distributed_amd.ops import _ext, dino
    assert dino.supported(N, D, K) and dino.splits(N, D, K) == tuple(_ext.require().dino_splits(N, D, K))


@pytest.mark.parametrize("N,D,K", [(40, 128, 320), (136, 128, 4096)])
def test_module_equals_op(gpu, N, D, K):
    """DINOLoss(backend="native") is the op, its centre the op's; frozen prototypes get a zero gradient."""
    from simclr_pytorch_distributed_amd.losses.dino import DINOLoss
    c = case(N, D, K, TEMPS[0], gpu)
    zs, zt, vs, vt, center = (t.to(gpu) for t in inputs(N, D, K))
    crit = DINOLoss(K, TEMPS[0], M_C, backend="native").to(gpu)
    crit.center.copy_(center)
    for frozen in (False, True):
        crit.set_frozen(frozen)
        zs.grad, vs.grad = None, None
        loss = crit(zs.requires_grad_(True), zt, vs.requires_grad_(True), vt)
        (G * loss).backward()
        want_dv = torch.zeros_like(c["runs"][0][2]) if frozen else c["runs"][0][2]
        for a, b in zip((loss.detach().reshape(1), zs.grad, vs.grad), (*c["runs"][0][:2], want_dv)):
            assert torch.equal(a.cpu(), b)
    crit.update_center()
    assert torch.equal(crit.center.cpu(), c["runs"][0][3])
    with pytest.raises(RuntimeError, match="unsupported shape"):
        crit(zs[:, :32], zt[:, :32], vs[:, :32], vt[:, :32])      # native never falls back
