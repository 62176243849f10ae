"""Supervised cross-entropy trainer (main_ce.py, engine/supervised.py) without a GPU: the
parser, the --label_frac subset, one epoch of the engine on the torch backend on the CPU, and
the torch form of the classifier + cross-entropy node."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def test_parse_ce_defaults_and_round_trip(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_ce
    opt = parse_ce(["--work_dir", str(tmp_path)], make_dirs=False)
    # the reference's main_ce.py recipe
    assert (opt.batch_size, opt.epochs, opt.learning_rate, opt.lr_decay_epochs) == (256, 500, 0.2, [350, 400, 450])
    assert (opt.weight_decay, opt.momentum, opt.model, opt.dataset, opt.size) == (1e-4, 0.9, "resnet50", "cifar10", 32)
    assert (opt.ckpt, opt.label_frac, opt.val_freq, opt.n_cls) == ("", 1.0, 1, 10)
    assert (opt.stem, opt.backend, opt.precision, opt.optimizer, opt.syncBN) == ("cifar", "auto", "bf16", "sgd", False)
    assert not opt.cosine and not opt.warm and opt.resume == ""
    assert opt.model_name.startswith("SupCE_cifar10_resnet50_lr_0.2")
    opt = parse_ce(["--work_dir", str(tmp_path), "--dataset", "cifar100", "--model", "resnet18", "--batch_size", "512",
                    "--epochs", "30", "--learning_rate", "0.05", "--cosine", "--syncBN", "--optimizer", "lars",
                    "--ckpt", "x.pth", "--label_frac", "0.1", "--val_freq", "5", "--stem", "imagenet",
                    "--backend", "torch", "--precision", "fp32", "--lr_decay_epochs", "10,20"], make_dirs=False)
    assert (opt.dataset, opt.model, opt.batch_size, opt.epochs, opt.learning_rate) == ("cifar100", "resnet18", 512, 30, 0.05)
    assert opt.cosine and opt.syncBN and opt.optimizer == "lars" and opt.ckpt == "x.pth"
    assert (opt.label_frac, opt.val_freq, opt.n_cls, opt.stem) == (0.1, 5, 100, "imagenet")
    assert (opt.backend, opt.precision, opt.lr_decay_epochs) == ("torch", "fp32", [10, 20])
    assert opt.warm and opt.warm_epochs == 10            # batch_size > 256 switches the warm-up on
    assert "frac_0.1" in opt.model_name and opt.model_name.endswith("_cosine_warm")
    assert parse_ce(["--n_cls", "7", "--work_dir", str(tmp_path)], make_dirs=False).n_cls == 7
    for bad in (["--label_frac", "0"], ["--label_frac", "1.5"], ["--cuda_graph"], ["--micro_batch", "8"],
                ["--val_freq", "0"]):
        with pytest.raises(ValueError):
            parse_ce(bad + ["--work_dir", str(tmp_path)], make_dirs=False)


def test_label_subset():
    from simclr_pytorch_distributed_amd.data.sampler import label_subset
    rng = np.random.default_rng(3)
    counts = [30, 7, 1, 101, 64]
    labels = rng.permutation(np.repeat(np.arange(5), counts))
    for num, den in ((1, 10), (1, 100), (1, 4), (1, 2)):
        f = num / den
        sub = label_subset(labels, f, seed=5)
        want = [(n * num + den - 1) // den for n in counts]          # ceil(f · n_c) in integers
        assert np.bincount(labels[sub], minlength=5).tolist() == want
        assert sub.size == sum(want) and np.unique(sub).size == sub.size and np.all(np.diff(sub) > 0)
        assert np.array_equal(sub, label_subset(labels, f, seed=5))
    a, b = label_subset(labels, 0.25, seed=5), label_subset(labels, 0.25, seed=6)
    assert a.size == b.size and not np.array_equal(a, b)
    assert np.array_equal(label_subset(labels, 1.0, seed=5), np.arange(labels.size))
    with pytest.raises(ValueError):
        label_subset(labels, 0.0)


def test_classifier_ce_torch_form():
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce, classifier_ce_logits
    torch.manual_seed(0)
    fc = torch.nn.Linear(64, 10)
    x = torch.randn(37, 64, requires_grad=True)
    y = torch.randint(0, 10, (37,))
    loss, stats = classifier_ce(x, fc, y)
    ref = F.cross_entropy(F.linear(x, fc.weight, fc.bias), y)
    assert torch.equal(loss, ref)
    gx, gw, gb = torch.autograd.grad(loss, [x, fc.weight, fc.bias])
    rx, rw, rb = torch.autograd.grad(ref, [x, fc.weight, fc.bias])
    assert torch.equal(gx, rx) and torch.equal(gw, rw) and torch.equal(gb, rb)
    logits = classifier_ce_logits(x, fc, y)[2]
    top5 = logits.topk(5, dim=1).indices
    assert not stats.requires_grad and not logits.requires_grad
    assert abs(float(stats[0]) - 37 * float(ref)) < 1e-4
    assert float(stats[1]) == float((top5[:, 0] == y).sum()) and float(stats[2]) == float((top5 == y[:, None]).sum())


def _ce_opt(tmp_path, *extra):
    from simclr_pytorch_distributed_amd.config import parse_ce
    return parse_ce(["--model", "resnet18", "--backend", "torch", "--dist_backend", "gloo", "--synthetic",
                     "--synthetic_size", "64", "--batch_size", "16", "--epochs", "1", "--learning_rate", "0.05",
                     "--print_freq", "2", "--save_freq", "1", "--val_batch_size", "500", "--work_dir", str(tmp_path),
                     *extra])


def test_supervised_engine_cpu_epoch(tmp_path):
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    torch.set_num_threads(4)
    opt = _ce_opt(tmp_path)
    eng = SupervisedEngine(opt, device=torch.device("cpu"))
    assert "fc.weight" in eng.flat.names and "fc.bias" in eng.flat.names
    assert eng.model.fc.weight.grad.data_ptr() >= eng.flat.grad.data_ptr()      # a view of the flat buffer
    w0 = eng.model.fc.weight.detach().clone()
    last = eng.run()
    assert os.path.basename(last) == "last.pth" and os.path.exists(last)
    assert os.path.exists(os.path.join(opt.save_folder, "ckpt_epoch_1.pth"))
    assert eng.global_step == 4 and len(eng.history) == 1                        # 64 images / 16
    h = eng.history[0]
    assert set(h) == {"epoch", "train_loss", "train_acc", "val_loss", "val_acc", "val_acc5"}
    assert math.isfinite(h["train_loss"]) and 0.0 < h["train_loss"] < 10.0 and math.isfinite(h["val_loss"])
    assert 0.0 <= h["train_acc"] <= 100.0 and 0.0 <= h["val_acc"] <= h["val_acc5"] <= 100.0
    assert not torch.equal(w0, eng.model.fc.weight.detach())                     # the optimizer owns fc
    st = ckpt_mod.load_checkpoint(last)
    assert set(st) == {"opt", "model", "optimizer", "epoch", "sdx_state"} and st["epoch"] == 1
    assert all(k.startswith("module.") for k in st["model"])
    assert "module.fc.weight" in st["model"] and "module.encoder.conv1.weight" in st["model"]
    m = SupCEResNet("resnet18", 10)
    ckpt_mod.load_model_state(m, st["model"])                                    # strict
    assert torch.equal(m.fc.weight, eng.model.fc.weight.detach())
    # --resume continues after the stored epoch
    eng2 = SupervisedEngine(_ce_opt(tmp_path, "--epochs", "2", "--resume", last), device=torch.device("cpu"))
    assert eng2.start_epoch == 2 and eng2.global_step == 4
    assert torch.equal(eng2.model.fc.weight.detach(), eng.model.fc.weight.detach())


def test_fine_tune_ckpt_and_label_frac_cpu(tmp_path):
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet, SupConResNet
    torch.manual_seed(11)
    src = SupConResNet("resnet18")
    path = str(tmp_path / "supcon.pth")
    torch.save({"opt": {}, "model": ckpt_mod.model_state_with_prefix(src), "optimizer": {}, "epoch": 1}, path)
    opt = _ce_opt(tmp_path, "--ckpt", path, "--label_frac", "0.5", "--seed", "0")
    eng = SupervisedEngine(opt, device=torch.device("cpu"))
    own = eng.model.state_dict()
    for k, v in src.encoder.state_dict().items():
        assert torch.equal(own["encoder." + k], v), k
    torch.manual_seed(opt.seed)
    fresh = SupCEResNet("resnet18", 10)
    assert torch.equal(own["fc.weight"], fresh.fc.weight) and torch.equal(own["fc.bias"], fresh.fc.bias)
    # the sampler runs over the class-balanced half
    n_c = np.bincount(eng._labels_np, minlength=10)
    assert eng.subset.size == int(np.sum((n_c + 1) // 2)) and eng.sampler.n == eng.subset.size
    seen = torch.cat([i for i, _ in eng.epoch_batches(1)]).tolist()
    assert set(seen) <= set(eng.subset.tolist())
    with pytest.raises(KeyError):
        bad = str(tmp_path / "nohead.pth")
        torch.save({"opt": {}, "model": {"module.fc.weight": torch.zeros(1)}, "optimizer": {}, "epoch": 1}, bad)
        SupervisedEngine(_ce_opt(tmp_path, "--ckpt", bad), device=torch.device("cpu"))


def test_set_loader_unchanged(monkeypatch):
    import argparse

    import main_ce
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    calls = []
    monkeypatch.setattr(main_ce, "build_dataset", lambda *a: calls.append(a) or ("ds", a[2]))
    opt = argparse.Namespace(dataset="cifar10", data_folder="./datasets/", synthetic=True)
    (tr, aug_tr), (va, aug_va) = main_ce.set_loader(opt)
    mean, std = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
    assert aug_tr == AugConfig.linear_train(32, mean, std) and aug_va == AugConfig.evaluation(32, mean, std)
    assert calls == [("cifar10", "./datasets/", True, True), ("cifar10", "./datasets/", False, True)]
    assert tr == ("ds", True) and va == ("ds", False)
    with pytest.raises(ValueError):
        main_ce.set_loader(argparse.Namespace(dataset="path", data_folder=".", synthetic=True))
    assert callable(main_ce.main)
