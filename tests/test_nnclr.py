"""NNCLR on the CPU: the plain-torch twin against a write-out of the paper's Algorithm 1 with Python loops,
the tie rule, the ring buffer's wrap-around, the flags, and one engine step with save / resume."""
import math

import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64


def test_reference_is_the_papers_loop():
    """Algorithm 1, symmetrised: nn = NN(z_v, Q), loss += CE(nn_v @ p̂_{1−v}.T / τ, arange) per view; loops over
    i and k in fp64. z gets no gradient."""
    from simclr_pytorch_distributed_amd.losses.moco import queue_value
    from simclr_pytorch_distributed_amd.losses.nnclr import NNCLRLoss
    n, D, K, T = 5, 16, 12, 0.1
    gen = torch.Generator().manual_seed(2)
    crit = NNCLRLoss(K, D, T, backend="torch", seed=4)
    Q = queue_value(crit.queue, F64)
    z = torch.randn(2 * n, D, generator=gen, dtype=F64).requires_grad_(True)
    p = torch.randn(2 * n, D, generator=gen, dtype=F64).requires_grad_(True)
    loss = crit(z, p)
    loss.backward()
    assert z.grad is None
    q = p.detach().clone().requires_grad_(True)
    zh, ph = F.normalize(z.detach(), dim=1).view(2, n, D), F.normalize(q, dim=1).view(2, n, D)
    want = 0.0
    for v in range(2):
        for i in range(n):
            sims = [float(zh[v, i] @ Q[j]) for j in range(K)]
            nbr = Q[max(range(K), key=lambda j: (sims[j], -j))]
            logits = [nbr @ ph[1 - v, k] / T for k in range(n)]
            want = want + torch.log(sum(torch.exp(x) for x in logits)) - logits[i]
    want = want / (2 * n)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    assert (p.grad - q.grad).abs().max() <= 1e-12 * q.grad.abs().max()


def test_ties_go_to_the_lower_index():
    from simclr_pytorch_distributed_amd.losses.nnclr import nn_index
    Q = F.normalize(torch.randn(9, 8, generator=torch.Generator().manual_seed(0), dtype=F64), dim=1)
    Q[7], Q[5] = Q[2], Q[0]                         # exact duplicates at higher indices
    assert nn_index(Q, Q).tolist() == [0, 1, 2, 3, 4, 0, 6, 2, 8]


def test_enqueue_wraps():
    from simclr_pytorch_distributed_amd.losses.nnclr import NNCLRLoss
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    n, D, K = 4, 8, 10
    crit = NNCLRLoss(K, D, backend="torch", seed=1)
    crit.ptr.fill_(8)                               # ptr + n > K
    want = crit.queue.clone()
    z = torch.randn(2 * n, D, generator=torch.Generator().manual_seed(3))
    crit(z, torch.randn(2 * n, D))
    crit.enqueue(z)
    want[:, (8 + torch.arange(n)) % K] = split_planes(F.normalize(z[n:], dim=1))      # view 1's rows
    assert torch.equal(crit.queue, want) and int(crit.ptr) == 2


def test_config():
    from simclr_pytorch_distributed_amd.config import NNCLR_DEFAULTS, parse_pretrain
    base = ["--model", "resnet18", "--synthetic"]
    opt = parse_pretrain(base + ["--method", "NNCLR", "--nnclr_k", "4096"], make_dirs=False)
    assert opt.method == "NNCLR" and opt.nnclr_k == 4096 and not hasattr(opt, "nnclr_temp")
    assert NNCLR_DEFAULTS == {"k": 98304, "temp": 0.1, "pred_hidden": 4096}
    assert not any(k.startswith("nnclr") for k in vars(parse_pretrain(base, make_dirs=False)))
    for flag, v in (("k", "4096"), ("temp", "0.2"), ("pred_hidden", "64")):
        with pytest.raises(ValueError, match="needs --method NNCLR"):
            parse_pretrain(base + ["--nnclr_" + flag, v], make_dirs=False)
    for flag in (["--micro_batch", "4"], ["--cuda_graph"]):
        with pytest.raises(ValueError, match=flag[0][2:]):
            parse_pretrain(base + ["--method", "NNCLR"] + flag, make_dirs=False)
    for bad in (["--nnclr_k", "64"], ["--nnclr_k", "4100"], ["--nnclr_temp", "0"], ["--nnclr_pred_hidden", "48"]):
        with pytest.raises(ValueError, match="nnclr_k"):     # below --batch_size, no multiple of 64, ...
            parse_pretrain(base + ["--method", "NNCLR"] + bad, make_dirs=False)


def test_engine_step_and_resume(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine import checkpoint as ck
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    args = ["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32", "--epochs", "1",
            "--max_steps", "1", "--backend", "torch", "--method", "NNCLR", "--nnclr_k", "64", "--nnclr_pred_hidden",
            "32", "--work_dir", str(tmp_path / "ws")]
    eng = PretrainEngine(parse_pretrain(args, make_dirs=True), device=torch.device("cpu"))
    assert not eng._momentum() and not any(k.startswith("predictor.") for k in SupConResNet("resnet18").state_dict())
    assert {k for k in eng.model.state_dict() if k.startswith("predictor.")} >= {"predictor.0.weight", "predictor.3.weight"}
    rows, forward = [], eng.criterion.forward
    eng.criterion.forward = lambda z, p: (rows.append(F.normalize(z.detach().float(), dim=1)), forward(z, p))[1]
    want, prev = eng.criterion.queue.clone(), eng.flat.flat.clone()
    st = eng.train_step(torch.arange(8), 1, 0, 1)
    assert math.isfinite(st["loss_local"].item()) and not torch.equal(eng.flat.flat, prev)
    assert eng.model.predictor[0].weight.grad is not None and eng.model.predictor[0].weight.grad.abs().sum() > 0
    want[:, :8] = split_planes(rows[0][8:])         # view 1's normalised projections
    assert torch.equal(eng.criterion.queue, want) and int(eng.criterion.ptr) == 8
    eng._save(1, "nnclr.pth")
    path = eng.opt.save_folder + "/nnclr.pth"
    st = ck.load_checkpoint(path)
    assert {"nnclr_queue", "nnclr_ptr"} <= set(st) and "model_k" not in st
    ropt = parse_pretrain(args + ["--resume", path], make_dirs=False)
    ropt.save_folder, ropt.tb_folder = eng.opt.save_folder, eng.opt.tb_folder
    res = PretrainEngine(ropt, device=torch.device("cpu"))
    assert torch.equal(res.flat.flat, eng.flat.flat)
    assert torch.equal(res.criterion.queue, eng.criterion.queue) and int(res.criterion.ptr) == 8
    # another method's run and its checkpoint know nothing of NNCLR; the probe takes this run's encoder
    other = PretrainEngine(parse_pretrain(args[:args.index("--method")] + ["--work_dir", str(tmp_path / "w2")],
                                          make_dirs=True), device=torch.device("cpu"))
    other._save(1, "simclr.pth")
    assert not {"nnclr_queue", "nnclr_ptr"} & set(ck.load_checkpoint(other.opt.save_folder + "/simclr.pth"))
    assert not hasattr(other.model, "predictor")
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    lopt = parse_linear(["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32",
                         "--epochs", "1", "--max_steps", "1", "--backend", "torch", "--ckpt", path,
                         "--work_dir", str(tmp_path / "lin")], make_dirs=True)
    le = LinearEngine(lopt, device=torch.device("cpu"))
    for (k, a), (_, b) in zip(eng.model.encoder.state_dict().items(), le.model.encoder.state_dict().items()):
        assert torch.equal(a, b), k
