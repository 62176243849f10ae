"""SwAV on the CPU: the plain-torch twin against a write-out of the official loop, the flags, the
model's prototype layer and a pretraining run whose checkpoint the linear probe loads."""
import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64


def official(z1, z2, C, eps, temp, iters):
    """The official two-crop loop: exp, Q /= sum, the transposed Sinkhorn iterations, Q *= B."""
    N = z1.shape[0]
    out = F.normalize(torch.cat([z1, z2]), dim=1) @ C.t()
    loss = 0
    for crop in range(2):
        with torch.no_grad():
            Q = torch.exp(out[N * crop:N * (crop + 1)] / eps).t()
            K, B = Q.shape
            Q /= Q.sum()
            for _ in range(iters):
                Q /= Q.sum(dim=1, keepdim=True)
                Q /= K
                Q /= Q.sum(dim=0, keepdim=True)
                Q /= B
            q = (Q * B).t()
        other = out[N * (1 - crop):N * (2 - crop)] / temp
        loss = loss - torch.mean(torch.sum(q * F.log_softmax(other, dim=1), dim=1))
    return loss / 2


@pytest.mark.parametrize("N,D,K", [(6, 8, 5), (16, 32, 40)])
def test_reference_is_the_official_loop(N, D, K):
    from simclr_pytorch_distributed_amd.losses import swav_reference
    gen = torch.Generator().manual_seed(N + K)
    z1, z2 = (torch.randn(N, D, generator=gen, dtype=F64) for _ in range(2))
    C = F.normalize(torch.randn(K, D, generator=gen, dtype=F64), dim=1)
    grads = []
    for fn in (official, swav_reference):
        leaves = [t.clone().requires_grad_(True) for t in (z1, z2, C)]
        loss = fn(*leaves, 0.05, 0.1, 3)
        grads.append([loss.detach(), *torch.autograd.grad(loss, leaves)])
    for a, b in zip(*grads):
        assert (a - b).abs().max() <= 1e-11 * max(1.0, a.abs().max().item())


def test_config():
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    base = ["--model", "resnet18", "--synthetic"]
    opt = parse_pretrain(base + ["--method", "SwAV", "--swav_prototypes", "200"], make_dirs=False)
    assert opt.method == "SwAV" and opt.swav_prototypes == 200 and not hasattr(opt, "swav_eps")
    assert not any(k.startswith("swav") for k in vars(parse_pretrain(base, make_dirs=False)))
    for flag, v in (("prototypes", "10"), ("eps", "0.05"), ("temp", "0.1"), ("iters", "3"), ("freeze_iters", "1")):
        with pytest.raises(ValueError, match="needs --method SwAV"):
            parse_pretrain(base + ["--swav_" + flag, v], make_dirs=False)
    with pytest.raises(ValueError, match="micro_batch"):
        parse_pretrain(base + ["--method", "SwAV", "--micro_batch", "4"], make_dirs=False)
    with pytest.raises(ValueError, match="swav_freeze_iters 0"):      # a captured step cannot end the freeze
        parse_pretrain(base + ["--method", "SwAV", "--cuda_graph"], make_dirs=False)
    assert parse_pretrain(base + ["--method", "SwAV", "--cuda_graph", "--swav_freeze_iters", "0"], make_dirs=False).cuda_graph


def test_prototype_layer_and_probe_load(tmp_path):
    """Two CPU steps of --method SwAV (the twin): the prototypes keep their direction while frozen and
    move afterwards; the run's checkpoint carries prototypes.weight and its encoder loads into the probe."""
    from simclr_pytorch_distributed_amd.config import parse_linear, parse_pretrain
    from simclr_pytorch_distributed_amd.engine import checkpoint as ck
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    assert "prototypes.weight" not in SupConResNet("resnet18").state_dict()
    opt = parse_pretrain(["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32",
                          "--epochs", "1", "--max_steps", "2", "--backend", "torch", "--method", "SwAV",
                          "--swav_prototypes", "12", "--swav_freeze_iters", "1",
                          "--work_dir", str(tmp_path / "ws")], make_dirs=True)
    eng = PretrainEngine(opt, device=torch.device("cpu"))
    w = eng.model.prototypes.weight
    assert w.shape == (12, 128)
    d0 = F.normalize(w.detach().clone(), dim=1)
    last = eng.run()
    d2 = F.normalize(w.detach(), dim=1)
    assert torch.isfinite(w).all() and (d2 - d0).abs().max() > 1e-6      # step 2 moved them
    sd = ck.strip_prefix(ck.load_checkpoint(last)["model"])
    assert sd["prototypes.weight"].shape == (12, 128)
    lopt = parse_linear(["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32",
                         "--epochs", "1", "--max_steps", "1", "--backend", "torch", "--ckpt", last,
                         "--work_dir", str(tmp_path / "lin")], make_dirs=True)
    le = LinearEngine(lopt, device=torch.device("cpu"))
    for (k, a), (_, b) in zip(eng.model.encoder.state_dict().items(), le.model.encoder.state_dict().items()):
        assert torch.equal(a, b), k


def test_frozen_prototypes_keep_their_direction():
    from simclr_pytorch_distributed_amd.losses import SwAVLoss
    gen = torch.Generator().manual_seed(3)
    C = torch.nn.Parameter(torch.randn(10, 16, generator=gen) * 3)
    crit = SwAVLoss(C, backend="torch")
    feats = torch.randn(12, 16, generator=gen, requires_grad=True)
    assert "_proto" not in dict(crit.named_parameters()) and not list(crit.parameters())
    crit.set_frozen(True)
    crit(feats).backward()
    assert C.grad is None and torch.allclose(C.detach().norm(dim=1), torch.ones(10), atol=1e-6)
    crit.set_frozen(False)
    crit(feats).backward()
    assert C.grad is not None and C.grad.abs().max() > 0
