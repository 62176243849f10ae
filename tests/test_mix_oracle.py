"""Mixup / CutMix / label smoothing without a GPU: the oracle against float64 torch, the draws,
the parser, the torch-backend engine step, and the fp32 twins of the kernels under the checks the
GPU tests apply (tests/mix_checks.py), where every named defect must be caught."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mix_checks as MC
import mix_oracle as MO

F64 = torch.float64


# ---- soft loss and gradient --------------------------------------------------------------------

@pytest.mark.parametrize("C,lam,eps", [(1, 1.0, 0.0), (3, 0.3, 0.1), (65, 0.5, 0.1), (1000, 0.0, 0.0), (5, 1.0, 0.1)])
def test_oracle_soft_loss_and_gradient_match_float64_torch(C, lam, eps):
    g = torch.Generator().manual_seed(C)
    B = 7
    z = (3.0 * torch.randn(B, C, generator=g, dtype=F64)).requires_grad_(True)
    a, b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    t = MO.soft_target(a, b, lam, eps, C)
    assert torch.allclose(t.sum(1), torch.ones(B, dtype=F64), atol=1e-15)
    ref = F.cross_entropy(z, t, reduction="none")
    got = MO.soft_ce(z.detach(), a, b, lam, eps, 1.0 / B)
    assert float((got["loss"] - ref.detach()).abs().max()) <= 1e-12
    (gz,) = torch.autograd.grad(ref.mean(), [z])
    assert float((got["dz"] - gz).abs().max()) <= 1e-12
    zz = z.detach()
    above = (zz > zz.gather(1, a[:, None])).sum(1)
    assert torch.equal(got["hit1"], (above < 1).to(F64)) and torch.equal(got["hit5"], (above < 5).to(F64))


def test_oracle_invalid_label_rows():
    z = torch.randn(4, 5, dtype=F64)
    got = MO.soft_ce(z, [0, -1, 2, 5], [1, 1, -1, 0], 0.3, 0.1, 0.25)
    assert torch.isnan(got["loss"]).tolist() == [False, True, True, True]
    assert got["hit1"][1:].sum() == 0 and got["hit5"][1:].sum() == 0
    assert torch.allclose(got["dz"][1:], 0.25 * torch.softmax(z[1:], 1), atol=1e-15)


def test_round_bf16_is_nearest_even():
    s = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -30, -3.0, 0.0, 257.0, 255.5], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.015625, 1.0078125, -3.0, 0.0, 256.0, 256.0])
    assert torch.equal(MO.round_bf16(s).float(), want)


# ---- draws -------------------------------------------------------------------------------------

def test_box_rule_is_torchvisions():
    from simclr_pytorch_distributed_amd.data.augment import cutmix_box
    MC.check_box(cutmix_box)
    with pytest.raises(AssertionError):
        MC.check_box(cutmix_box, defect="lam_uncorrected")


def _mix_opt(**kw):
    return argparse.Namespace(**dict(dict(mixup=0.8, cutmix=1.0, mix_prob=1.0, mix_switch_prob=0.5, size=32), **kw))


def test_mix_draw_deterministic_rank_dependent_and_off():
    from simclr_pytorch_distributed_amd.data.augment import mix_draw
    opt = _mix_opt()
    draws = [mix_draw(opt, 3, e, it, 0) for e in (1, 2) for it in range(40)]
    assert draws == [mix_draw(opt, 3, e, it, 0) for e in (1, 2) for it in range(40)]
    assert draws != [mix_draw(opt, 3, e, it, 1) for e in (1, 2) for it in range(40)]
    assert draws != [mix_draw(opt, 4, e, it, 0) for e in (1, 2) for it in range(40)]
    modes = [d[0] for d in draws]
    assert set(modes) == {"mixup", "cutmix"}
    for mode, lam, (y0, y1, x0, x1) in draws:
        assert 0.0 <= lam <= 1.0 and 0 <= y0 <= y1 <= 32 and 0 <= x0 <= x1 <= 32
        if mode == "cutmix":
            assert lam == 1.0 - (y1 - y0) * (x1 - x0) / 1024
    off = _mix_opt(mixup=0.0, cutmix=0.0)
    assert all(mix_draw(off, 3, 1, it, 0)[0] == "none" for it in range(50))
    assert all(mix_draw(_mix_opt(mix_prob=0.0), 3, 1, it, 0)[0] == "none" for it in range(50))
    assert {mix_draw(_mix_opt(cutmix=0.0), 3, 1, it, 0)[0] for it in range(50)} == {"mixup"}
    assert {mix_draw(_mix_opt(mixup=0.0), 3, 1, it, 0)[0] for it in range(50)} == {"cutmix"}
    assert {mix_draw(_mix_opt(mix_switch_prob=1.0), 3, 1, it, 0)[0] for it in range(50)} == {"cutmix"}
    half = [mix_draw(_mix_opt(mix_prob=0.5), 3, 1, it, 0)[0] for it in range(200)]
    assert 60 <= half.count("none") <= 140


# ---- parser ------------------------------------------------------------------------------------

def test_parser_flags_absent_change_nothing(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_ce
    base = ["--work_dir", str(tmp_path), "--model", "resnet18"]
    opt = parse_ce(base, make_dirs=False)
    for k in ("label_smoothing", "mixup", "cutmix", "mix_prob", "mix_switch_prob"):
        assert k not in vars(opt)
    assert (opt.label_smoothing, opt.mixup, opt.cutmix, opt.mix_prob, opt.mix_switch_prob) == (0.0, 0.0, 0.0, 1.0, 0.5)
    assert opt.model_name == "SupCE_cifar10_resnet18_lr_0.2_decay_0.0001_bsz_256_trial_0"
    on = parse_ce(base + ["--label_smoothing", "0.1", "--mixup", "0.8", "--cutmix", "1.0"], make_dirs=False)
    assert on.model_name == opt.model_name + "_ls_0.1_mixup_0.8_cutmix_1.0"
    assert (vars(on)["label_smoothing"], vars(on)["mixup"], vars(on)["cutmix"]) == (0.1, 0.8, 1.0)
    assert parse_ce(base + ["--label_smoothing", "0.1"], make_dirs=False).save_folder != opt.save_folder
    p = parse_ce(base + ["--cutmix", "1", "--mix_prob", "0.5"], make_dirs=False)
    assert p.model_name.endswith("_cutmix_1.0_mixp_0.5")


@pytest.mark.parametrize("bad", [["--label_smoothing", "1.0"], ["--label_smoothing", "-0.1"], ["--mixup", "-1"],
                                 ["--cutmix", "nan"], ["--cutmix", "inf"], ["--mix_prob", "1.5"],
                                 ["--mix_switch_prob", "-0.5"]])
def test_parser_refuses_bad_values(tmp_path, bad):
    from simclr_pytorch_distributed_amd.config import parse_ce
    with pytest.raises(SystemExit):
        parse_ce(["--work_dir", str(tmp_path)] + bad, make_dirs=False)


@pytest.mark.parametrize("parse", ["parse_pretrain", "parse_linear"])
def test_other_trainers_do_not_take_the_flags(tmp_path, parse):
    import simclr_pytorch_distributed_amd.config as cfg
    with pytest.raises(SystemExit):
        getattr(cfg, parse)(["--work_dir", str(tmp_path), "--mixup", "0.8"], make_dirs=False)


# ---- torch form of the node and of the mixing ---------------------------------------------------

def test_classifier_ce_torch_form_soft():
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce_logits
    torch.manual_seed(0)
    fc = torch.nn.Linear(64, 10)
    x = torch.randn(9, 64)
    a, b = torch.randint(0, 10, (9,)), torch.randint(0, 10, (9,))
    loss, stats, logits = classifier_ce_logits(x, fc, a, labels2=b, lam=0.3, smoothing=0.1)
    ref = MO.soft_ce(logits, a, b, 0.3, 0.1, 1.0 / 9)
    assert abs(float(loss.detach()) - float(ref["loss"].mean())) < 5e-6         # fp32 torch on 10 classes
    assert float(stats[1]) == float(ref["hit1"].sum()) and float(stats[2]) == float(ref["hit5"].sum())
    plain = classifier_ce_logits(x, fc, a)
    same = classifier_ce_logits(x, fc, a, labels2=None, lam=1.0, smoothing=0.0)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1], same[1])
    with pytest.raises(ValueError):
        classifier_ce_logits(x, fc, a, lam=1.5)


def test_mix_reference_matches_oracle():
    from simclr_pytorch_distributed_amd.data.augment import mix_reference
    x = MC.batch(5, 7)
    for name, box in MC.boxes(7).items():
        MC.check_cutmix(mix_reference(x, "cutmix", 0.5, box, "nhwc"), x, box, name)
        nchw = x.permute(0, 3, 1, 2).contiguous()
        got = mix_reference(nchw, "cutmix", 0.5, box)
        MC.check_cutmix(got.permute(0, 2, 3, 1).contiguous(), x, box, name + " nchw")
    MC.check_mixup_wide(mix_reference(x, "mixup", 0.3, layout="nhwc"), x, 0.3)
    xe = MC.batch(2, 7, exact=True)
    for lam in (0.25, 0.5, 0.75):
        MC.check_mixup_exact(mix_reference(xe, "mixup", lam, layout="nhwc"), xe, lam)


# ---- the twins under the GPU tests' checks; every defect is caught ------------------------------

def _twin_mix(defect=None):
    return lambda x, mode, lam, box: MC.mix_twin(x, mode, lam, box, defect)


def _twin_ce(defect=None):
    return lambda z, a, b, lam, eps, g: MC.soft_twin(z, a, b, lam, eps, g, defect)


def test_twins_pass_every_case():
    for name in MC.MIX_CASES:
        MC.run_mix_case(_twin_mix(), name)
    worst = MC.Worst()
    for name in MC.CE_CASES:
        MC.run_ce_case(_twin_ce(), name, worst)
    print(f"soft CE twin: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("defect,case", [("partner_next", "partner"), ("box_inclusive", "box_end"),
                                         ("lam_after_rounding", "one_rounding")])
def test_mix_defect_is_caught(defect, case):
    assert defect in MC.MIX_DEFECTS
    with pytest.raises(AssertionError):
        MC.run_mix_case(_twin_mix(defect), case)


@pytest.mark.parametrize("defect,case", [("smooth_c_minus_1", "smooth"), ("second_label_unsmoothed", "two_labels"),
                                         ("hits_b", "hits"), ("no_gscale", "gscale")])
def test_ce_defect_is_caught(defect, case):
    assert defect in MC.CE_DEFECTS
    with pytest.raises(AssertionError):
        MC.run_ce_case(_twin_ce(defect), case)


# ---- engine, torch backend ----------------------------------------------------------------------

def _engine(tmp_path, *extra):
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    opt = parse_ce(["--model", "resnet18", "--backend", "torch", "--dist_backend", "gloo", "--synthetic",
                    "--synthetic_size", "16", "--batch_size", "8", "--epochs", "1", "--learning_rate", "0.05",
                    "--val_batch_size", "16", "--work_dir", str(tmp_path), "--seed", "1", *extra])
    return SupervisedEngine(opt, device=torch.device("cpu"))


def _plain_step_body(self, idx, labels, epoch=1, it=0):
    """The step body as it was before the soft-target code: the bypass."""
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
    zeroed, x = self._start_step(idx, epoch, it)
    feat = self.runner.encode(x)
    loss, stats = classifier_ce(feat, self.model.fc, labels, native=False, gemm=self.head_gemm())
    self._backward_and_update(loss, zeroed)
    return {"loss_local": loss.detach(), "stats": stats}


def test_engine_step_reports_the_hand_mixed_loss(tmp_path):
    from simclr_pytorch_distributed_amd.data import augment as A
    torch.set_num_threads(4)
    eng = _engine(tmp_path, "--mixup", "0.8", "--cutmix", "1.0", "--label_smoothing", "0.1")
    eng.model.train()
    seen = set()
    for it, (idx, labels) in enumerate(eng.epoch_batches(1)):
        mode, lam, box = A.mix_draw(eng.opt, eng.opt.seed, 1, it, 0)
        seen.add(mode)
        eng._host_prelude(1, it, 2)
        x = eng.make_views(idx, 1, it)                       # NCHW fp32, the step's own views
        xr = x.roll(1, 0)
        if mode == "cutmix":
            y0, y1, x0, x1 = box
            inside = torch.zeros(1, 1, 32, 32, dtype=torch.bool)
            inside[:, :, y0:y1, x0:x1] = True
            xm = torch.where(inside, xr, x)
        else:
            xm = np.float32(lam) * x + (np.float32(1) - np.float32(lam)) * xr
        t = MO.soft_target(labels, labels.roll(1), lam, 0.1, eng.opt.n_cls).float()
        with torch.no_grad():
            logits = eng.model.fc(eng.runner.encode(xm).float())
            want = F.cross_entropy(logits, t)
            dom = labels if lam >= 0.5 else labels.roll(1)
            hits = float(((logits > logits.gather(1, dom[:, None])).sum(1) < 1).sum())
        st = eng.train_step(idx, labels, 1, it, 2)
        assert abs(float(st["loss_local"]) - float(want)) <= 2e-6 * max(1.0, abs(float(want))), (it, mode)
        assert float(st["stats"][1]) == hits
    assert seen <= {"mixup", "cutmix"} and seen


def test_engine_flags_absent_is_bit_identical_to_the_bypass(tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    torch.set_num_threads(4)
    a = _engine(tmp_path / "a")
    monkeypatch.setattr(SupervisedEngine, "_mix", lambda *args: pytest.fail("the mixing code ran with the flags absent"))
    b = _engine(tmp_path / "b")
    monkeypatch.setattr(b, "_step_body", _plain_step_body.__get__(b))
    assert torch.equal(a.flat.flat, b.flat.flat)
    for eng in (a, b):
        eng.model.train()
    (ia, la), (ib, lb) = next(iter(a.epoch_batches(1))), next(iter(b.epoch_batches(1)))
    sa, sb = a.train_step(ia, la, 1, 0, 2), b.train_step(ib, lb, 1, 0, 2)
    assert torch.equal(sa["loss_local"], sb["loss_local"]) and torch.equal(sa["stats"], sb["stats"])
    assert torch.equal(a.flat.flat, b.flat.flat)
