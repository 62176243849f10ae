"""MoCo on the CPU: the plain-torch twin against a write-out of the official loop over a wrapping
queue, the flags, and three engine steps (the key encoder's EMA, the ring buffer, save / resume)."""
import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64


def test_reference_is_the_official_loop():
    """moco/builder.py: cat([l_pos, l_neg]) / T, cross_entropy with label 0, _dequeue_and_enqueue
    (slots per row, so the ring may wrap mid-batch: K = 2.5 batches, three steps)."""
    from simclr_pytorch_distributed_amd.losses.moco import MoCoLoss, queue_value
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    N, D, K, T = 4, 16, 10, 0.2
    gen = torch.Generator().manual_seed(5)
    crit = MoCoLoss(K, D, T, backend="torch", seed=3)
    queue = queue_value(crit.queue, F64).t().clone()     # [D][K], as the official buffer
    assert (queue.norm(dim=0) - 1).abs().max() < 2.0 ** -17     # hi + lo keeps 2^-18 of an element
    ptr = 0
    for step in range(3):
        q0, k0 = (torch.randn(N, D, generator=gen, dtype=F64) for _ in range(2))
        res = []
        for ours in (False, True):
            q = q0.clone().requires_grad_(True)
            if ours:
                loss = crit(q, k0)
            else:
                qn, kn = F.normalize(q, dim=1), F.normalize(k0, dim=1)
                l_pos = torch.einsum("nc,nc->n", qn, kn).unsqueeze(-1)
                l_neg = torch.einsum("nc,ck->nk", qn, queue.clone().detach())
                logits = torch.cat([l_pos, l_neg], dim=1) / T
                loss = F.cross_entropy(logits, torch.zeros(N, dtype=torch.long))
            res.append((loss.detach(), torch.autograd.grad(loss, q)[0]))
        for a, b in zip(*res):
            assert (a - b).abs().max() <= 1e-11 * max(1.0, a.abs().max().item()), step
        crit.enqueue(k0)
        keys = queue_value(split_planes(F.normalize(k0.float(), dim=1)), F64)    # what the planes hold
        for i in range(N):
            queue[:, (ptr + i) % K] = keys[i]
        ptr = (ptr + N) % K
        assert int(crit.ptr) == ptr and torch.equal(queue_value(crit.queue, F64), queue.t()), step
    assert ptr == 2     # wrapped inside the third batch


def test_config():
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    base = ["--model", "resnet18", "--synthetic"]
    opt = parse_pretrain(base + ["--method", "MoCo", "--moco_k", "4096"], make_dirs=False)
    assert opt.method == "MoCo" and opt.moco_k == 4096 and not hasattr(opt, "moco_m")
    assert not any(k.startswith("moco") for k in vars(parse_pretrain(base, make_dirs=False)))
    for flag, v in (("k", "4096"), ("m", "0.99"), ("temp", "0.2")):
        with pytest.raises(ValueError, match="needs --method MoCo"):
            parse_pretrain(base + ["--moco_" + flag, v], make_dirs=False)
    for flag in (["--micro_batch", "4"], ["--cuda_graph"]):
        with pytest.raises(ValueError, match=flag[0][2:]):
            parse_pretrain(base + ["--method", "MoCo"] + flag, make_dirs=False)
    with pytest.raises(ValueError, match="moco_k"):
        parse_pretrain(base + ["--method", "MoCo", "--moco_k", "64"], make_dirs=False)     # below --batch_size


def test_engine_steps_and_resume(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.ops.moco import split_planes
    args = ["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32", "--epochs", "1",
            "--max_steps", "3", "--backend", "torch", "--method", "MoCo", "--moco_k", "20", "--moco_m", "0.9",
            "--work_dir", str(tmp_path / "ws")]
    eng = PretrainEngine(parse_pretrain(args, make_dirs=True), device=torch.device("cpu"))
    assert not any(p.requires_grad for p in eng.model_k.parameters())
    assert torch.equal(eng.flat_k.flat, eng.flat.flat) and eng.flat_k.flat.data_ptr() != eng.flat.flat.data_ptr()
    keys, enqueue = [], eng.criterion.enqueue
    eng.criterion.enqueue = lambda k: (keys.append(F.normalize(k.detach().float(), dim=1)), enqueue(k))[1]
    want = eng.criterion.queue.clone()
    for it in range(3):
        q_prev, k_prev = eng.flat.flat.clone(), eng.flat_k.flat.clone()
        st = eng.train_step(torch.arange(8 * it, 8 * it + 8), 1, it, 3)
        assert torch.isfinite(st["loss_local"]).item()
        assert torch.equal(eng.flat_k.flat, k_prev.mul(0.9).add(q_prev, alpha=1.0 - 0.9))     # the EMA recurrence
        assert not torch.equal(eng.flat.flat, q_prev)
        for i in range(8):
            want[:, (8 * it + i) % 20] = split_planes(keys[it])[:, i]
    assert torch.equal(eng.criterion.queue, want) and int(eng.criterion.ptr) == 24 % 20
    eng._save(1, "moco.pth")
    ropt = parse_pretrain(args + ["--resume", eng.opt.save_folder + "/moco.pth"], make_dirs=False)
    ropt.save_folder, ropt.tb_folder = eng.opt.save_folder, eng.opt.tb_folder
    res = PretrainEngine(ropt, device=torch.device("cpu"))
    for (n, a), (_, b) in zip(eng.model_k.state_dict().items(), res.model_k.state_dict().items()):
        assert torch.equal(a, b), n
    assert torch.equal(res.flat.flat, eng.flat.flat)
    assert torch.equal(res.criterion.queue, eng.criterion.queue) and int(res.criterion.ptr) == 4
