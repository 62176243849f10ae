"""The MoCo kernels (csrc/kernels/moco.hip, ema_update of optim.hip) on the GPU, stage by stage against
fp64, every stage's reference evaluated on the kernel's OWN inputs to that stage (its q̂, k̂ and l⁺, its
lse, its slabs), as test_gpu_swav.py does. The queue's value is hi + lo of its planes, exactly.

u = 2^-24; "1.01" covers second-order terms; IT = fp32(1/T).

enqueue bit-exact: hi = bf16(x), lo = bf16(x − hi) at slots (ptr + i) mod K, the other rows untouched.
ema     both products and the sum in fp64, rounded once: u·|result| <= the issue's 2u·(|m·p_k| + |(1 − m)·p_q|).
prep    rn = fp32(1/‖x‖): u·rn. x̂ = fl(x·rn): 2.02u·|x̂|. l⁺: an fp64 dot of the kernel's q̂, k̂ rounded once.
S       (2^-16 + D·u)·Σ|q̂||Q|, the GEMM bound of test_gpu_vicreg.py =: B_S; in logits B_S·IT.
exp/log __expf(x) = exp(x)(1 + δ), |δ| <= K_EXP·(1 + |x|)·u and __logf(l) = log l + ε, |ε| <= K_LOG·(1 + |log l|)·u,
        the constants test_gpu_swav.py measured (tools/explog_probe, |x| <= 30.3) and doubled. The forward's
        arguments are x − max with |x − max| <= 2·IT <= 28.6, inside that range. The backward forms
        s·IT − lse, which could reach −2·IT − log(K + 1) = −36.9 at T = 0.07, K = 4096, so the probe was
        re-run on the backward's own arguments at these shapes (tools/explog_probe/measure_moco.py,
        profiles/moco.txt): they lie in [−19.95, −0.02] and the worst |δ| is 1.1634·(1 + |x|)·u, so twice
        that (2.33) is within K_EXP. exp_err asserts that every argument it is given stays within 30.3.
lse     logits off by B_S·IT + 3u·IT (fl(s·IT), fl(x − max)), weighted by the softmax; every term's exp
        K_EXP·(1 + 2·IT)·u; the running sum is rescaled when the max moves, at most C = span tiles + 2
        shuffles + splits + 1 times, the moves adding up to <= 2·IT: K_EXP·(C + 2·IT)·u; A = 8·span tiles +
        2 + splits + 1 fp32 additions of positive terms: A·u; L = fl(max + __logf(l)): K_LOG·(1 + log l)·u + u·|L|.
loss    fp64 sum of fl(l⁺·IT) − lse over the kernel's lse, rounded once: u·Σ|l⁺·IT|/N + 1.01·u·|L|.
slabs   p = __expf(fma(s, IT, −lse)): δp = p*·(B_S·IT + e(arg)); the product Pᵀ·Q: (2^-16 + K·u)·Σ p*|Q|.
dq      splits fp32 additions and the positive term (p⁺ − 1)·k̂, scaled by fl(g·fp32(1/(N·T))) (3u), then
        fl(fl(v − q̂·t)·rn), t the fp32 of an fp64 dot: 4u·(|v| + |q̂|·Σ|q̂·v|)·rn, the error of v carried through.

End to end the tolerances are test_gpu_vicreg.py's: 1e-4 of the loss, 1e-3 of the largest gradient element.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import headgemm_checks as CK
from aux_oracle import f32_value

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = CK.U
EPS_P = 2.0 ** -16
K_EXP, K_LOG = 2.38, 3.68       # test_gpu_swav.py: twice the worst measured
PROBED = 30.3
# one tile pair and one split with a ragged row block; ragged rows and spans (10 tiles in spans of 4, 4, 2);
# several row blocks and splits; the largest D
SHAPES = [(8, 64, 64), (40, 128, 320), (264, 128, 4096), (64, 256, 1024)]
TEMPS = [0.2, 0.07]
G = 1.7
WORST = CK.Worst()


def inputs(N, D, K, seed=0):
    """q, k: row norms spread over two decades, k correlated with q; the queue: normalised rows as planes."""
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    gen = torch.Generator().manual_seed(seed + 31 * N + D + K)
    q, k = (torch.randn(N, D, generator=gen, dtype=F64) * 10.0 ** (2 * torch.rand(N, 1, generator=gen, dtype=F64) - 1)
            for _ in range(2))
    k = k + 0.7 * q
    rows = F.normalize(torch.randn(K, D, generator=gen, dtype=F64), dim=1)
    rows[: min(K, N)] += 0.8 * F.normalize(q[: min(K, N)], dim=1)      # some hard negatives
    return q.float(), k.float(), split_planes(F.normalize(rows, dim=1).float())


_CASE = {}


def case(N, D, K, T, dev):
    """The kernels' stage outputs (fp64 CPU tensors), computed once per shape and temperature."""
    if (N, D, K, T) not in _CASE:
        from simclr_pytorch_distributed_amd.ops import _ext
        m = _ext.require()
        q, k, queue = (t.to(dev) for t in inputs(N, D, K))
        loss, lse, lpos, qhat, rq, khat = m.moco_fwd(q, k, queue, T, 0)
        dq, slab = m.moco_bwd(qhat, rq, khat, queue, lse, lpos, torch.tensor([G], device=dev), T, 0)
        torch.cuda.synchronize()
        o = dict(q=q, k=k, loss=loss, lse=lse, lpos=lpos, qhat=qhat, rq=rq, khat=khat, dq=dq, slab=slab)
        _CASE[N, D, K, T] = dict({n: v.cpu().to(F64) for n, v in o.items()}, splits=m.moco_splits(N, D, K),
                                 Q=(queue[0].cpu().to(F64) + queue[1].cpu().to(F64)))
    return _CASE[N, D, K, T]


def exp_err(x):
    assert x.abs().max().item() <= PROBED, "an __expf argument outside the probed range: re-run the probe"
    return (K_EXP * (1 + x.abs()) + 2 * x.abs()) * U


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("N,D,K", SHAPES)
def test_forward(gpu, N, D, K, T):
    c = case(N, D, K, T, gpu)
    ctx = f"[N={N} D={D} K={K} T={T}]"
    IT = f32_value(1 / T)
    for x, xh in ((c["q"], c["qhat"]), (c["k"], c["khat"])):
        ref = x / x.norm(dim=1, keepdim=True)
        CK.within(WORST, "xhat", xh, ref, 2.02 * U * ref.abs(), ctx)
    rn = 1 / c["q"].norm(dim=1)
    CK.within(WORST, "rq", c["rq"], rn, U * rn, ctx)
    lp = (c["qhat"] * c["khat"]).sum(1)
    CK.within(WORST, "lpos", c["lpos"], lp, U * lp.abs() + 1e-14, ctx)
    qh, Q, S_ = c["qhat"], c["Q"], c["splits"]
    from simclr_pytorch_distributed_amd.ops import moco
    assert moco.supported(N, D, K) and moco.splits(N, K) == S_, f"{ctx} the Python mirror of moco_plan.h"
    logits = torch.cat([c["lpos"][:, None], qh @ Q.t()], 1) * IT
    B_S = torch.cat([torch.zeros(N, 1, dtype=F64), (EPS_P + D * U) * (qh.abs() @ Q.abs().t())], 1) * IT
    lse = torch.logsumexp(logits, 1)
    p = (logits - lse[:, None]).exp()
    span = -(-(K // 32) // S_)
    C, A = span + 2 + S_ + 1, 8 * span + 2 + S_ + 1
    logl = lse - logits.max(1).values
    B = 1.01 * ((p * B_S).sum(1) + 3 * U * IT + (K_EXP * (1 + 2 * IT) + K_EXP * (C + 2 * IT) + A) * U) \
        + K_LOG * (1 + logl) * U + U * lse.abs()
    CK.within(WORST, "lse", c["lse"], lse, B, ctx)
    x = c["lpos"] * IT
    loss = -(x - c["lse"]).sum() / N
    CK.within(WORST, "loss", c["loss"], loss.reshape(1), (U * x.abs().sum() / N + 1.01 * U * loss.abs()).reshape(1), ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("N,D,K", SHAPES)
def test_backward(gpu, N, D, K, T):
    c = case(N, D, K, T, gpu)
    ctx = f"[N={N} D={D} K={K} T={T}]"
    IT = f32_value(1 / T)
    qh, kh, Q, S_, slab = c["qhat"], c["khat"], c["Q"], c["splits"], c["slab"]
    assert slab.shape == (S_, N, D)
    arg = (qh @ Q.t()) * IT - c["lse"][:, None]
    p = arg.exp()
    dp = 1.01 * p * ((EPS_P + D * U) * (qh.abs() @ Q.abs().t()) * IT + exp_err(arg))
    CK.within(WORST, "slabs", slab.sum(0), p @ Q, dp @ Q.abs() + (EPS_P + K * U) * (p @ Q.abs()), ctx)
    argp = c["lpos"] * IT - c["lse"]
    pm1 = argp.exp() - 1
    a = slab.sum(0) + pm1[:, None] * kh
    Ba = S_ * U * (slab.abs().sum(0) + (pm1[:, None] * kh).abs()) + (argp.exp() * exp_err(argp) + U)[:, None] * kh.abs()
    sc = f32_value(G) * f32_value(1 / (N * T))
    v, rn = a * sc, c["rq"][:, None]
    Bv = 1.01 * (sc * Ba + 3 * U * v.abs())
    dq = (v - qh * (qh * v).sum(1, keepdim=True)) * rn
    B = rn * (Bv + qh.abs() * (qh.abs() * Bv).sum(1, keepdim=True)) \
        + 4 * U * rn * (v.abs() + qh.abs() * (qh * v).abs().sum(1, keepdim=True))
    CK.within(WORST, "dq", c["dq"], dq, 1.01 * B, ctx)
    print(ctx, WORST.report())


@pytest.mark.parametrize("N,D,K,ptr", [(40, 128, 320, 300), (8, 64, 64, 60), (64, 256, 1024, 0)])
def test_enqueue_bit_exact(gpu, N, D, K, ptr):
    from simclr_pytorch_distributed_amd.ops import moco
    _, k, queue = inputs(N, D, K)
    keys = F.normalize(k, dim=1)
    got, p = queue.to(gpu), torch.tensor([ptr], device=gpu)
    moco.enqueue(got, p, keys.to(gpu))
    want = queue.clone()
    want[:, (ptr + torch.arange(N)) % K] = moco.split_planes(keys)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)) and p.item() == (ptr + N) % K


def test_ema_update(gpu):
    from simclr_pytorch_distributed_amd.ops import moco
    n, m = 4096 * 256 * 4 + 4 * 1000 + 3, 0.999       # past one pass of the 4096 x 256 grid, n % 4 = 3
    gen = torch.Generator().manual_seed(1)
    pk, pq = (torch.randn(n, generator=gen) for _ in range(2))
    got = pk.to(gpu)
    moco.ema_update(got, pq.to(gpu), m)
    a, b = m * pk.to(F64), (1 - m) * pq.to(F64)
    CK.within(WORST, "ema", got.cpu(), a + b, 2 * U * (a.abs() + b.abs()), "[ema]")


@pytest.mark.parametrize("N,D,K", [(40, 128, 320), (264, 128, 4096)])
def test_module_end_to_end(gpu, N, D, K):
    """MoCoLoss (native) against fp64 autograd of the twin; two launches are bit-identical."""
    from simclr_pytorch_distributed_amd.losses.moco import MoCoLoss, moco_reference
    q, k, queue = inputs(N, D, K, seed=7)
    crit = MoCoLoss(K, D, 0.07, backend="native").to(gpu)
    crit.queue.copy_(queue)
    runs = []
    for _ in range(2):
        x = q.to(gpu).requires_grad_(True)
        loss = crit(x, k.to(gpu))
        (G * loss).backward()
        runs.append((loss.detach().reshape(1), x.grad))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    a = q.to(F64).requires_grad_(True)
    ref = moco_reference(a, k.to(F64), queue, 0.07)
    (G * ref).backward()
    assert abs(runs[0][0].item() - ref.item()) <= 1e-4 * abs(ref.item())
    err = (runs[0][1].cpu().to(F64) - a.grad).abs().max().item()
    print(f"e2e dq err/max {err / a.grad.abs().max().item():.3g}")
    assert err <= 1e-3 * a.grad.abs().max().item()
    # enqueue(k) of the tensor the forward took stores the k̂ that moco_prep formed, bit for bit
    from simclr_pytorch_distributed_amd.ops import _ext, moco
    kg = k.to(gpu)
    loss = crit(q.to(gpu).requires_grad_(True), kg)
    khat = _ext.require().moco_prep(q.to(gpu), kg)[2]
    assert not torch.equal(khat, F.normalize(kg, dim=1))      # else the comparison below shows nothing
    crit.enqueue(kg)
    assert crit.ptr.item() == N % K
    assert torch.equal(crit.queue[:, :N].view(torch.int16), moco.split_planes(khat).view(torch.int16))
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()      # the queue it saved has been written since


def test_engine_step(gpu, tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    opt = parse_pretrain(["--method", "MoCo", "--moco_k", "128", "--moco_m", "0.9", "--model", "resnet18", "--synthetic",
                          "--synthetic_size", "64", "--batch_size", "32", "--feat_dim", "128", "--max_steps", "2",
                          "--backend", "native", "--work_dir", str(tmp_path)], make_dirs=False)
    eng = PretrainEngine(opt)
    for it in range(opt.max_steps):
        q_prev, k_prev = eng.flat.flat.clone(), eng.flat_k.flat.clone()
        st = eng.train_step(torch.arange(32 * it, 32 * it + 32, device=gpu), 1, it, 2)
        assert torch.isfinite(st["loss_local"]).item()
        want = 0.9 * k_prev.to(F64) + (1 - 0.9) * q_prev.to(F64)
        assert (eng.flat_k.flat.to(F64) - want).abs().max().item() <= U * want.abs().max().item()
    assert eng.criterion.ptr.item() == 64 and math.isfinite(eng.criterion.queue.float().sum().item())
    rows = eng.criterion.queue[:, :64].float().sum(0).norm(dim=1)
    assert (rows - 1).abs().max().item() < 1e-4
