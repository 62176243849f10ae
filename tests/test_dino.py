"""DINO on the CPU: the plain-torch twin against a write-out of the official loss and centre update, the
flags, and one engine step (the teacher's EMA, the checkpoint's keys)."""
import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64


def test_reference_is_the_official_loop():
    """dino/main_dino.py DINOLoss.forward + update_center with ncrops = 2 behind DINOHead's last layer
    (normalize, then weight_norm with g = 1); two steps, so the second sees a non-zero centre."""
    from simclr_pytorch_distributed_amd.losses.dino import DINOLoss
    N, D, K, ts, tt, mc = 5, 16, 12, 0.1, 0.04, 0.9
    gen = torch.Generator().manual_seed(11)
    crit = DINOLoss(K, (ts, tt), mc, backend="torch").double()
    center = torch.zeros(1, K, dtype=F64)
    for step in range(2):
        zs0, zt0 = (torch.randn(2 * N, D, generator=gen, dtype=F64) for _ in range(2))
        vs0, vt0 = (torch.randn(K, D, generator=gen, dtype=F64) * (1 + torch.arange(K, dtype=F64)[:, None])
                    for _ in range(2))
        res = []
        for ours in (False, True):
            zs, vs = zs0.clone().requires_grad_(True), vs0.clone().requires_grad_(True)
            if ours:
                loss = crit(zs, zt0, vs, vt0)
            else:
                student_output = F.normalize(zs, dim=-1) @ (vs / vs.norm(dim=1, keepdim=True)).t()
                teacher_output = F.normalize(zt0, dim=-1) @ (vt0 / vt0.norm(dim=1, keepdim=True)).t()
                student_out = (student_output / ts).chunk(2)
                teacher_out = F.softmax((teacher_output - center) / tt, dim=-1).detach().chunk(2)
                total_loss, n_loss_terms = 0, 0
                for iq, q in enumerate(teacher_out):
                    for v in range(len(student_out)):
                        if v == iq:
                            continue
                        total_loss += torch.sum(-q * F.log_softmax(student_out[v], dim=-1), dim=-1).mean()
                        n_loss_terms += 1
                loss = total_loss / n_loss_terms
                batch_center = torch.sum(teacher_output, dim=0, keepdim=True) / len(teacher_output)
                center = center * mc + batch_center.detach() * (1 - mc)
            res.append((loss.detach(), *torch.autograd.grad(loss, (zs, vs))))
        crit.update_center()
        for a, b in zip(*res):
            assert (a - b).abs().max() <= 1e-11 * max(1.0, a.abs().max().item()), step
        assert (crit.center - center[0]).abs().max() <= 1e-13 and center.abs().max() > 1e-3, step


def test_config():
    from simclr_pytorch_distributed_amd.config import DINO_DEFAULTS, parse_pretrain
    base = ["--model", "resnet18", "--synthetic"]
    opt = parse_pretrain(base + ["--method", "DINO", "--dino_prototypes", "4096"], make_dirs=False)
    assert opt.method == "DINO" and opt.dino_prototypes == 4096 and not hasattr(opt, "dino_m")
    assert (DINO_DEFAULTS["prototypes"], DINO_DEFAULTS["student_temp"], DINO_DEFAULTS["teacher_temp"],
            DINO_DEFAULTS["warmup_teacher_temp"], DINO_DEFAULTS["warmup_epochs"], DINO_DEFAULTS["m"],
            DINO_DEFAULTS["center_m"]) == (65536, 0.1, 0.04, 0.04, 0, 0.996, 0.9)
    assert not any(k.startswith("dino") for k in vars(parse_pretrain(base, make_dirs=False)))
    for flag, v in (("prototypes", "64"), ("student_temp", "0.1"), ("teacher_temp", "0.04"), ("center_m", "0.9"),
                    ("warmup_teacher_temp", "0.04"), ("warmup_epochs", "1"), ("m", "0.99"), ("freeze_iters", "3")):
        with pytest.raises(ValueError, match="needs --method DINO"):
            parse_pretrain(base + ["--dino_" + flag, v], make_dirs=False)
    for flag in (["--micro_batch", "4"], ["--cuda_graph"]):
        with pytest.raises(ValueError, match=flag[0][2:]):
            parse_pretrain(base + ["--method", "DINO"] + flag, make_dirs=False)


def test_engine_step_and_checkpoint(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    common = ["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "16", "--epochs", "1",
              "--max_steps", "1", "--backend", "torch", "--work_dir", str(tmp_path / "ws")]
    args = common + ["--method", "DINO", "--dino_prototypes", "24", "--dino_m", "0.9", "--dino_freeze_iters", "0"]
    eng = PretrainEngine(parse_pretrain(args, make_dirs=True), device=torch.device("cpu"))
    assert not any(p.requires_grad for p in eng.model_k.parameters())
    assert torch.equal(eng.flat_k.flat, eng.flat.flat) and eng.flat_k.flat.data_ptr() != eng.flat.flat.data_ptr()
    s_prev, t_prev = eng.flat.flat.clone(), eng.flat_k.flat.clone()
    proto_prev = eng.model.prototypes.weight.detach().clone()
    st = eng.train_step(torch.arange(8), 1, 0, 2)
    assert torch.isfinite(st["loss_local"]).item() and eng._dino_m == 0.9
    assert not torch.equal(eng.flat.flat, s_prev) and not torch.equal(eng.model.prototypes.weight, proto_prev)
    # official order: the teacher follows the UPDATED student, θ_t += (1 − m)·(θ_s − θ_t)
    assert torch.equal(eng.flat_k.flat, t_prev.mul(0.9).add(eng.flat.flat, alpha=1.0 - 0.9))
    assert eng.criterion.center.abs().max().item() > 0
    eng._save(1, "dino.pth")
    st = torch.load(eng.opt.save_folder + "/dino.pth", weights_only=False)
    assert "model_k" in st and torch.equal(st["dino_center"], eng.criterion.center)
    ref = PretrainEngine(parse_pretrain(common, make_dirs=True), device=torch.device("cpu"))
    ref._save(1, "simclr.pth")
    other = torch.load(ref.opt.save_folder + "/simclr.pth", weights_only=False)
    assert not {"model_k", "dino_center"} & set(other) and not hasattr(ref.model, "prototypes")
