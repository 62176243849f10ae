"""CPU tests of knowledge distillation for the supervised trainer (--distill_ckpt): the fp64 oracle
against float64 torch autograd of the stock-op form, the fp32 twin and its defect matrix under the
derived bounds (tests/distill_checks.py), the torch form of ``classifier_ce``, the parser, and a
torch-backend engine with a ResNet-18 teacher checkpoint the test writes itself.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_checks as DC
import distill_oracle as DO
import mix_checks as MC
import mix_oracle as MO


# ---- oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,lam,eps,temp,alpha", [(1, 1.0, 0.0, 2.0, 0.5), (3, 0.3, 0.1, 0.5, 0.5), (65, 0.5, 0.1, 4.0, 0.25),
                                                  (1000, 1.0, 0.0, 2.0, 1.0), (5, 1.0, 0.1, 1.0, 0.0)])
def test_oracle_loss_and_gradient_match_float64_torch(C, lam, eps, temp, alpha):
    B = 7
    g = torch.Generator().manual_seed(C)
    z = (3 * torch.randn(B, C, generator=g, dtype=torch.float64)).requires_grad_(True)
    v = 3 * torch.randn(B, C, generator=g, dtype=torch.float64)
    a, b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    t = MO.soft_target(a, b, lam, eps, C)
    kd = F.kl_div(F.log_softmax(z / temp, 1), F.softmax(v / temp, 1), reduction="batchmean") * temp * temp
    loss = (1 - alpha) * F.cross_entropy(z, t) + alpha * kd
    grad, = torch.autograd.grad(loss, [z])
    it, tau = DO.temperature(temp)                      # (powers of two: it = 1 / τ exactly)
    R = DO.distill_ce(z.detach(), v, a, b, lam, eps, it, tau, alpha, 1.0 / B)
    loss = loss.detach()
    assert abs(float(R["loss"].mean()) - float(loss)) < 1e-12 * max(1.0, abs(float(loss)))
    assert float((R["dz"] - grad).abs().max()) < 1e-13
    assert bool((R["kd"] >= -1e-12).all())              # a KL divergence


def test_oracle_label_rules():
    z, v = torch.randn(4, 5, dtype=torch.float64), torch.randn(4, 5, dtype=torch.float64)
    a, b = torch.tensor([0, -1, 2, 5]), torch.tensor([1, 1, -1, 0])
    half = DO.distill_ce(z, v, a, b, 0.5, 0.0, 0.5, 2.0, 0.5, 0.25)
    assert torch.isnan(half["loss"]).tolist() == [False, True, True, True]
    assert half["hit5"].tolist() == [1.0, 0.0, 0.0, 0.0]
    # the invalid rows' dz carries no target term: (1 − α)·p + α·τ·(q_s − q_t)
    want = (0.5 * torch.softmax(z, 1) + 0.5 * 2.0 * (torch.softmax(z * 0.5, 1) - torch.softmax(v * 0.5, 1))) * 0.25
    assert torch.allclose(half["dz"][1:], want[1:], atol=1e-15)
    one = DO.distill_ce(z, v, a, b, 0.5, 0.0, 0.5, 2.0, 1.0, 0.25)
    assert not torch.isnan(one["loss"]).any() and torch.equal(one["loss"], one["kd"])
    assert one["hit5"].tolist() == [1.0, 0.0, 0.0, 0.0]
    same = DO.distill_ce(z, z, a, b, 0.5, 0.0, 0.5, 2.0, 1.0, 0.25)
    assert float(same["kd"].abs().max()) < 1e-15 and float(same["dz"].abs().max()) == 0.0


# ---- twin and defects ---------------------------------------------------------------------------

def _twin(defect=None):
    return lambda *args: DC.distill_twin(*args, defect=defect)


def test_twin_passes_every_case():
    worst = MC.Worst()
    for name in DC.CASES:
        DC.run_case(_twin(), name, worst)
    print(f"distill twin: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("defect", DC.DEFECTS)
def test_defect_is_caught_by_its_case(defect):
    assert defect in DC.CASES
    with pytest.raises(AssertionError):
        DC.run_case(_twin(defect), defect)


def test_teacher_rows_cover_the_kinds():
    z = torch.randn(5, 65)
    assert torch.equal(DC.teacher_rows(z, "equal"), z)
    p = DC.teacher_rows(z, "perm")
    assert torch.equal(p.sort(1).values, z.sort(1).values) and not torch.equal(p, z)
    assert set(DC.teacher_rows(z, "peaky").unique().tolist()) == {-40.0, 40.0}
    assert DC.teacher_rows(z, "const").unique().numel() == 1
    cold = [c for c in DC.CASES.values() if c[6] < 1.0]
    assert {c[5] for c in cold} >= {"equal", "perm", "peaky", "const"}


# ---- torch form of the node ---------------------------------------------------------------------

def test_classifier_ce_torch_form_distill():
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce, classifier_ce_logits
    torch.manual_seed(0)
    fc = torch.nn.Linear(64, 10)
    x = torch.randn(9, 64)
    a, b = torch.randint(0, 10, (9,)), torch.randint(0, 10, (9,))
    v = (3 * torch.randn(9, 10)).requires_grad_(True)
    for temp, alpha in ((2.0, 0.5), (0.5, 1.0), (1.0, 0.25)):
        loss, stats, logits = classifier_ce_logits(x, fc, a, labels2=b, lam=0.3, smoothing=0.1, teacher_logits=v,
                                                   temp=temp, alpha=alpha)
        it, tau = DO.temperature(temp)
        ref = DO.distill_ce(logits, v.detach(), a, b, 0.3, 0.1, it, tau, alpha, 1.0 / 9)
        assert abs(float(loss.detach()) - float(ref["loss"].mean())) < 1e-5
        assert abs(float(stats[0]) - float(ref["loss"].sum())) < 1e-4
        assert float(stats[1]) == float(ref["hit1"].sum()) and float(stats[2]) == float(ref["hit5"].sum())
        fc.zero_grad()
        loss.backward()
        assert v.grad is None                                                   # the teacher is a constant
        dW = ref["dz"].t() @ x.double()
        assert float((fc.weight.grad.double() - dW).abs().max()) < 1e-5
    # α = 1 with unlabelled rows: the loss is the kd term, no hit; α < 1 keeps refusing them
    un = torch.full((9,), -1)
    un[0] = int(logits[0].argmax())
    loss, stats = classifier_ce(x, fc, un, native=False, teacher_logits=v, temp=2.0, alpha=1.0)
    ref = DO.distill_ce(logits, v.detach(), un, un, 1.0, 0.0, 0.5, 2.0, 1.0, 1.0 / 9)
    assert abs(float(loss.detach()) - float(ref["kd"].mean())) < 1e-5 and stats.tolist()[1:] == [1.0, 1.0]
    with pytest.raises(Exception):
        classifier_ce(x, fc, un, native=False, teacher_logits=v, temp=2.0, alpha=0.5)
    # without a teacher the call is the one it was
    plain = classifier_ce_logits(x, fc, a)
    same = classifier_ce_logits(x, fc, a, teacher_logits=None, temp=3.0, alpha=0.5)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    for kw in (dict(temp=0.0), dict(temp=float("inf")), dict(alpha=1.5), dict(alpha=-0.1)):
        with pytest.raises(ValueError):
            classifier_ce_logits(x, fc, a, teacher_logits=v, **kw)
    with pytest.raises(ValueError):
        classifier_ce_logits(x, fc, a, teacher_logits=v[:, :5])


# ---- parser -------------------------------------------------------------------------------------

DISTILL_KEYS = ("distill_ckpt", "distill_model", "distill_temp", "distill_alpha")


def test_parser_flags_absent_change_nothing(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_ce
    base = ["--work_dir", str(tmp_path), "--model", "resnet18"]
    opt = parse_ce(base, make_dirs=False)
    assert not any(k in vars(opt) for k in DISTILL_KEYS)
    assert (opt.distill_ckpt, opt.distill_model, opt.distill_temp, opt.distill_alpha) == ("", None, 1.0, 1.0)
    assert opt.model_name == "SupCE_cifar10_resnet18_lr_0.2_decay_0.0001_bsz_256_trial_0"
    on = parse_ce(base + ["--distill_ckpt", "t.pth"], make_dirs=False)
    assert (on.distill_ckpt, on.distill_model, on.distill_temp, on.distill_alpha) == ("t.pth", "resnet18", 1.0, 1.0)
    assert on.model_name == opt.model_name + "_distill_resnet18_T_1.0_a_1.0"
    assert {k: v for k, v in vars(on).items() if k not in DISTILL_KEYS + ("model_name", "save_folder", "tb_folder")} \
        == {k: v for k, v in vars(opt).items() if k not in ("model_name", "save_folder", "tb_folder")}
    full = parse_ce(base + ["--distill_ckpt", "t.pth", "--distill_model", "resnet50", "--distill_temp", "4",
                            "--distill_alpha", "0.5", "--label_frac", "0.1"], make_dirs=False)
    assert (full.distill_model, full.distill_temp, full.distill_alpha) == ("resnet50", 4.0, 0.5)


@pytest.mark.parametrize("bad", [["--distill_ckpt", "t.pth", "--distill_temp", "0"],
                                 ["--distill_ckpt", "t.pth", "--distill_temp", "-1"],
                                 ["--distill_ckpt", "t.pth", "--distill_temp", "inf"],
                                 ["--distill_ckpt", "t.pth", "--distill_temp", "nan"],
                                 ["--distill_ckpt", "t.pth", "--distill_alpha", "1.5"],
                                 ["--distill_ckpt", "t.pth", "--distill_alpha", "-0.1"],
                                 ["--distill_ckpt", "t.pth", "--distill_alpha", "nan"],
                                 ["--distill_ckpt", ""],
                                 ["--distill_model", "resnet50"], ["--distill_temp", "2"], ["--distill_alpha", "0.5"]])
def test_parser_refuses_bad_values_and_dependent_flags_alone(tmp_path, bad):
    from simclr_pytorch_distributed_amd.config import parse_ce
    with pytest.raises(SystemExit):
        parse_ce(["--work_dir", str(tmp_path)] + bad, make_dirs=False)


@pytest.mark.parametrize("parse", ["parse_pretrain", "parse_linear"])
@pytest.mark.parametrize("flag", [["--distill_ckpt", "t.pth"], ["--distill_temp", "2"]])
def test_other_trainers_do_not_take_the_flags(tmp_path, parse, flag):
    import simclr_pytorch_distributed_amd.config as cfg
    with pytest.raises(SystemExit):
        getattr(cfg, parse)(["--work_dir", str(tmp_path)] + flag, make_dirs=False)


# ---- engine, torch backend ----------------------------------------------------------------------

def _engine(tmp_path, *extra):
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    opt = parse_ce(["--model", "resnet18", "--backend", "torch", "--dist_backend", "gloo", "--synthetic",
                    "--synthetic_size", "16", "--batch_size", "8", "--epochs", "1", "--learning_rate", "0.05",
                    "--val_batch_size", "16", "--save_freq", "1", "--work_dir", str(tmp_path), "--seed", "1", *extra])
    return SupervisedEngine(opt, device=torch.device("cpu"))


def _teacher_ckpt(path, n_cls=10, seed=5):
    """A ResNet-18 main_ce.py checkpoint (the reference's 4-key layout) with non-trivial BN statistics."""
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = SupCEResNet("resnet18", n_cls)
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        torch.save({"opt": {}, "model": ckpt_mod.model_state_with_prefix(model), "optimizer": {}, "epoch": 1}, str(path))
    return model


@pytest.fixture(scope="module")
def teacher_path(tmp_path_factory):
    p = tmp_path_factory.mktemp("teacher") / "teacher.pth"
    _teacher_ckpt(p)
    return str(p)


def _spy_node(monkeypatch):
    """Record (student logits, keyword arguments) of every classifier_ce call of the engine."""
    from simclr_pytorch_distributed_amd.engine import supervised as sup
    from simclr_pytorch_distributed_amd.ops import ce_head
    calls = []

    def spy(feat, fc, labels, native=True, gemm="fma", **kw):
        loss, stats, logits = ce_head.classifier_ce_logits(feat, fc, labels, native, gemm, **kw)
        calls.append((logits, labels, kw))
        return loss, stats

    monkeypatch.setattr(sup, "classifier_ce", spy)
    return calls


@pytest.mark.parametrize("extra", [("--distill_temp", "2", "--distill_alpha", "0.5", "--mixup", "0.8", "--label_smoothing", "0.1"),
                                   ("--distill_temp", "0.5", "--label_frac", "0.5")])
def test_engine_step_loss_is_the_oracle_on_the_spied_logits(tmp_path, teacher_path, monkeypatch, extra):
    torch.set_num_threads(4)
    eng = _engine(tmp_path, "--distill_ckpt", teacher_path, *extra)
    calls = _spy_node(monkeypatch)
    teacher_before = {k: v.clone() for k, v in eng.teacher.state_dict().items()}
    assert not eng.teacher.training and not any(p.requires_grad for p in eng.teacher.parameters())
    student = {id(p) for p in eng.model.parameters()}
    assert not any(id(p) in student for p in eng.teacher.parameters())
    lo, hi = eng.flat.flat.data_ptr(), eng.flat.flat.data_ptr() + 4 * eng.flat.flat.numel()
    assert all(lo <= p.data_ptr() < hi for p in eng.model.parameters())
    assert not any(lo <= p.data_ptr() < hi for p in eng.teacher.parameters())   # outside the flat buffer
    eng.model.train()
    alpha, temp = eng.distill_alpha, eng.distill_temp
    for it, (idx, labels) in enumerate(eng.epoch_batches(1)):
        st = eng.train_step(idx, labels, 1, it, 2)
        logits, lab, kw = calls[-1]
        v = kw["teacher_logits"]
        assert v.shape == logits.shape and not v.requires_grad and (kw["temp"], kw["alpha"]) == (temp, alpha)
        itv, tau = DO.temperature(temp)
        ref = DO.distill_ce(logits, v, lab, kw.get("labels2", lab), kw.get("lam", 1.0), kw.get("smoothing", 0.0),
                            itv, tau, alpha, 1.0 / 8)
        want = float(ref["loss"].mean())
        assert abs(float(st["loss_local"]) - want) <= 5e-6 * max(1.0, abs(want)), it
        assert float(st["stats"][1]) == float(ref["hit1"].sum())
    assert len(calls) == 2
    for k, v in eng.teacher.state_dict().items():
        assert torch.equal(v, teacher_before[k]), k                      # bit-unchanged, BN statistics included
    eng._save(1, "ckpt_epoch_1.pth")
    import os
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    saved = ckpt_mod.load_checkpoint(os.path.join(eng.opt.save_folder, "ckpt_epoch_1.pth"))
    assert set(ckpt_mod.strip_prefix(saved["model"])) == set(eng.model.state_dict())
    assert not any("teacher" in k for k in saved["model"])


def test_engine_teacher_sees_the_students_views(tmp_path, teacher_path, monkeypatch):
    """The teacher's logits are its own eval-mode forward of the step's (mixed) views."""
    torch.set_num_threads(4)
    eng = _engine(tmp_path, "--distill_ckpt", teacher_path)
    calls = _spy_node(monkeypatch)
    eng.model.train()
    idx, labels = next(iter(eng.epoch_batches(1)))
    eng._host_prelude(1, 0, 2)
    x = eng.make_views(idx, 1, 0)
    with torch.no_grad():
        want = eng.teacher(x)
    eng.train_step(idx, labels, 1, 0, 2)
    assert torch.allclose(calls[-1][2]["teacher_logits"], want, atol=1e-5)


def test_engine_refuses_a_teacher_of_another_width(tmp_path):
    p = tmp_path / "t7.pth"
    _teacher_ckpt(p, n_cls=7)
    with pytest.raises(ValueError, match=r"7 classes.*n_cls = 10"):
        _engine(tmp_path, "--distill_ckpt", str(p))


def test_alpha_one_samples_the_whole_store(tmp_path, teacher_path):
    whole = _engine(tmp_path / "a", "--distill_ckpt", teacher_path, "--label_frac", "0.1")
    assert whole.subset.size == len(whole.train) and np.array_equal(whole.subset, np.arange(len(whole.train)))
    part = _engine(tmp_path / "b", "--distill_ckpt", teacher_path, "--label_frac", "0.5", "--distill_alpha", "0.5")
    plain = _engine(tmp_path / "c", "--label_frac", "0.5")
    assert part.subset.size < len(part.train) and np.array_equal(part.subset, plain.subset)


def test_engine_flags_absent_is_bit_identical_to_the_bypass(tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
    torch.set_num_threads(4)
    a = _engine(tmp_path / "a")
    assert a.teacher is None
    monkeypatch.setattr(SupervisedEngine, "_teacher_logits", lambda *args: pytest.fail("the teacher ran"))
    b = _engine(tmp_path / "b")

    def body(idx, labels, epoch=1, it=0):
        zeroed, x = b._start_step(idx, epoch, it)
        loss, stats = classifier_ce(b.runner.encode(x), b.model.fc, labels, native=False, gemm=b.head_gemm())
        b._backward_and_update(loss, zeroed)
        return {"loss_local": loss.detach(), "stats": stats}

    monkeypatch.setattr(b, "_step_body", body)
    assert torch.equal(a.flat.flat, b.flat.flat)
    for eng in (a, b):
        eng.model.train()
    (ia, la), (ib, lb) = next(iter(a.epoch_batches(1))), next(iter(b.epoch_batches(1)))
    sa, sb = a.train_step(ia, la, 1, 0, 2), b.train_step(ib, lb, 1, 0, 2)
    assert torch.equal(sa["loss_local"], sb["loss_local"]) and torch.equal(sa["stats"], sb["stats"])
    assert torch.equal(a.flat.flat, b.flat.flat)
