"""The NNCLR kernels (csrc/kernels/nnclr.hip) on the GPU against fp64: the queue search exactly (seeded
inputs whose fp64 top-1 / top-2 gap exceeds 1e-4 on every row, and planted rows at the edges of the queue
and of a split span), the loss and its gradient at the project's end-to-end tolerances (test_gpu_moco.py,
test_gpu_vicreg.py): 1e-4 of lse and of the loss, 1e-3 of the largest gradient element. The queue's value is
hi + lo of its planes, exactly.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
F64 = torch.float64
# one row and one tile pair; a ragged row block and spans of three tiles; two row blocks per view, the
# largest D and 32 splits; 10 tiles in spans of 4, 4, 2
SHAPES = [(1, 64, 64), (5, 64, 192), (70, 256, 4096), (64, 128, 320)]
TEMPS = [0.1, 0.5]
G = 1.7
GAP = 1e-4
SEED = {(70, 256, 4096): 1}     # chosen on the CPU so that every row's gap exceeds GAP; 0 elsewhere


def inputs(n, D, K, N=None, seed=None):
    """z [2n][D], p [2][N][D] (row norms spread over two decades, correlated with z where it has a partner)
    and the queue: row-normalised Gaussian rows as planes."""
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    N = N or n
    seed = SEED.get((n, D, K), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(seed + 31 * n + D + K)
    z = F.normalize(torch.randn(2 * n, D, generator=gen, dtype=F64), dim=1).float()
    p = torch.randn(2, N, D, generator=gen, dtype=F64)
    p = p * 10.0 ** (2 * torch.rand(2, N, 1, generator=gen, dtype=F64) - 1)
    queue = split_planes(F.normalize(torch.randn(K, D, generator=gen, dtype=F64), dim=1).float())
    return z, p.float(), queue


def exact_search(z, queue, twice=None):
    """(idx, Q) in fp64, every row's top-1 / top-2 gap above GAP: no row is excused. Row ``twice`` has its
    best row in the queue two times: its gap is that to the third."""
    from simclr_pytorch_distributed_amd.losses.moco import queue_value
    from simclr_pytorch_distributed_amd.losses.nnclr import nn_index
    Q = queue_value(queue.cpu(), F64)
    zh = F.normalize(z.cpu().to(F64), dim=1)
    top = (zh @ Q.t()).topk(3, dim=1).values
    second = top[:, 1].clone()
    if twice is not None:
        assert top[twice, 0] == top[twice, 1]
        second[twice] = top[twice, 2]
    assert (top[:, 0] - second).min().item() > GAP
    return nn_index(zh, Q), Q


def ext():
    from simclr_pytorch_distributed_amd.ops import _ext
    return _ext.require()


@pytest.mark.parametrize("n,D,K", SHAPES)
def test_search(gpu, n, D, K):
    z, _, queue = (t.to(gpu) for t in inputs(n, D, K))
    want, _ = exact_search(z, queue)
    m = ext()
    idx, sim, nnpl = m.nnclr_search(m.nnclr_prep(z)[1], queue)
    assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), want)
    assert torch.equal(nnpl.view(torch.int16), queue[:, idx.long()].view(torch.int16))
    from simclr_pytorch_distributed_amd.ops import nnclr
    i2, s2 = nnclr.nn_search(z, queue)
    assert torch.equal(i2, idx) and torch.equal(s2, sim)
    assert nnclr.supported(n, D, K) and [nnclr.splits(n, K), nnclr.span(n, K)] == m.nnclr_splits(n, n, D, K)[:2]


@pytest.mark.parametrize("where", ["first", "last", "span_first", "span_last", "duplicate"])
def test_search_planted(gpu, where):
    """The best row of query r sits at an edge; an exact duplicate at a higher index in another span loses."""
    from simclr_pytorch_distributed_amd.losses.moco import queue_value
    from simclr_pytorch_distributed_amd.ops import nnclr
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    n, D, K = 70, 256, 4096
    z, _, queue = inputs(n, D, K)
    S, span = nnclr.splits(n, K), nnclr.span(n, K)
    assert S >= 3 and span % 32 == 0
    at = {"first": [0], "last": [K - 1], "span_first": [span], "span_last": [2 * span - 1],
          "duplicate": [span + 5, 3 * span + 9]}[where]
    r = 2 * n - 1                                   # a row of the ragged last block
    rows = queue_value(queue)
    rows[at] = z[r]
    queue = split_planes(rows)
    want, _ = exact_search(z, queue, r if where == "duplicate" else None)
    assert want[r].item() == at[0]
    m = ext()
    idx, _, nnpl = m.nnclr_search(m.nnclr_prep(z.to(gpu))[1], queue.to(gpu))
    assert torch.equal(idx.cpu().long(), want)
    assert torch.equal(nnpl.cpu().view(torch.int16), queue[:, want].view(torch.int16))


def check_loss(gpu, n, D, K, T, N=None, off=0):
    from simclr_pytorch_distributed_amd.losses.nnclr import nnclr_reference
    z, p, queue = inputs(n, D, K, N)
    idx64, Q = exact_search(z, queue)
    m = ext()
    zg, pg, qg = z.to(gpu), p.to(gpu).view(-1, D), queue.to(gpu)
    loss, lse, idx, _, _, nnpl, ppl, rp = m.nnclr_fwd(zg, pg, qg, T, off)
    dp, _ = m.nnclr_bwd(nnpl, ppl, pg, rp, lse, torch.tensor([G], device=gpu), T, off)
    assert torch.equal(idx.cpu().long(), idx64)
    a = p.to(F64).requires_grad_(True)
    ref = nnclr_reference(z.to(F64), None, queue, T, off, a)
    (G * ref).backward()
    ph, nbr = F.normalize(a.detach(), dim=2), Q[idx64].view(2, n, D)
    lse64 = torch.cat([torch.logsumexp(nbr[v] @ ph[1 - v].t() / T, dim=1) for v in range(2)])
    e_lse = ((lse.cpu().to(F64) - lse64).abs() / lse64.abs()).max().item()
    # N = 1: lse is the positive logit itself, so the loss and its gradient are 0 identically; the loss's error
    # is then held against the lse it is the remainder of
    s_loss = abs(ref.item()) or lse64.abs().mean().item()
    e_loss = abs(loss.item() - ref.item()) / s_loss
    d_dp, s_dp = (dp.cpu().to(F64).view_as(a) - a.grad).abs().max().item(), a.grad.abs().max().item()
    print(f"[n={n} N={N or n} D={D} K={K} T={T}] lse {e_lse:.3g} loss {e_loss:.3g} dp {d_dp:.3g} of max {s_dp:.3g}")
    assert e_lse <= 1e-4 and e_loss <= 1e-4 and d_dp <= 1e-3 * s_dp


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("n,D,K", SHAPES)
def test_forward_backward(gpu, n, D, K, T):
    check_loss(gpu, n, D, K, T)


def test_rows_of_a_gathered_batch(gpu):
    """n < N and pos_offset != 0: this rank's 32 rows per view against gathered predictions of 2 x 96 rows,
    the gradient for all of them."""
    check_loss(gpu, 32, 128, 320, 0.1, N=96, off=32)


def test_autograd_and_bit_identity(gpu):
    from simclr_pytorch_distributed_amd.ops import nnclr
    n, D, K = 70, 256, 4096
    z, p, queue = (t.to(gpu) for t in inputs(n, D, K))
    runs = []
    for _ in range(2):
        a, b = z.clone().requires_grad_(True), p.view(-1, D).clone().requires_grad_(True)
        loss, _, idx = nnclr.nnclr_loss_rows(a, b, queue, 0.1)
        (G * loss).backward()
        assert a.grad is None or not a.grad.any()
        runs.append((loss.detach().reshape(1).view(torch.int32), idx, b.grad.view(torch.int32)))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_module_end_to_end(gpu):
    """NNCLRLoss (native): forward, backward and enqueue; the written slots are nnclr_prep's ẑ of view 1."""
    from simclr_pytorch_distributed_amd.losses.nnclr import NNCLRLoss, nnclr_reference
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    n, D, K = 64, 128, 320
    z, p, queue = inputs(n, D, K, seed=7)
    crit = NNCLRLoss(K, D, 0.1, backend="native").to(gpu)
    crit.queue.copy_(queue)
    zg, pg = z.to(gpu) * 3.0, p.view(-1, D).to(gpu).requires_grad_(True)
    loss = crit(zg, pg)
    loss.backward()
    a = p.view(-1, D).to(F64).requires_grad_(True)
    ref = nnclr_reference(z.to(F64), a, queue, 0.1)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    assert (pg.grad.cpu().to(F64) - a.grad).abs().max().item() <= 1e-3 * a.grad.abs().max().item()
    zhat = ext().nnclr_prep(zg)[0]
    assert not torch.equal(zhat, F.normalize(zg, dim=1))      # else the comparison below shows nothing
    crit.enqueue(zg)
    assert crit.ptr.item() == n
    assert torch.equal(crit.queue[:, :n].view(torch.int16), split_planes(zhat[n:]).view(torch.int16))
    assert torch.equal(crit.queue[:, n:].cpu().view(torch.int16), queue[:, n:].view(torch.int16))


def test_engine_step(gpu, tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    opt = parse_pretrain(["--method", "NNCLR", "--nnclr_k", "128", "--nnclr_pred_hidden", "64", "--model", "resnet18",
                          "--synthetic", "--synthetic_size", "64", "--batch_size", "32", "--feat_dim", "128",
                          "--max_steps", "2", "--backend", "native", "--work_dir", str(tmp_path)], make_dirs=False)
    eng = PretrainEngine(opt)
    w0 = eng.model.predictor[0].weight.detach().clone()
    for it in range(opt.max_steps):
        st = eng.train_step(torch.arange(32 * it, 32 * it + 32, device=gpu), 1, it, 2)
        assert torch.isfinite(st["loss_local"]).item()
    assert not torch.equal(eng.model.predictor[0].weight, w0)
    assert eng.criterion.ptr.item() == 64 and math.isfinite(eng.criterion.queue.float().sum().item())
    rows = eng.criterion.queue[:, :64].float().sum(0).norm(dim=1)
    assert (rows - 1).abs().max().item() < 1e-4
