"""Linear-probe sweep (--sweep_lr / --sweep_wd) without a GPU: the parser, the per-head
learning-rate schedule, and the torch-path sweep of LinearEngine against single runs."""
import datetime

import pytest
import torch

from simclr_pytorch_distributed_amd.config import parse_linear, sweep_head_opts
from simclr_pytorch_distributed_amd.optim.schedules import lr_at_epoch, warmup_lr

NOW = datetime.datetime(2026, 10, 15, 21, 5)

# the attributes parse_linear set before the sweep flags existed
PLAIN_KEYS = {
    "backend", "batch_size", "ckpt", "comm_timeout", "conf_work_path", "cosine", "cuda_graph", "data_folder",
    "dataset", "dist_backend", "epochs", "feat_dim", "gpu_aug", "head", "knn", "knn_k", "knn_t", "learning_rate",
    "local_rank", "lr_decay_epochs", "lr_decay_rate", "max_steps", "mean", "mean_t", "model", "model_name",
    "model_path", "momentum", "n_cls", "num_workers", "precision", "print_freq", "profile", "rank", "resize",
    "save_folder", "save_freq", "seed", "size", "std", "std_t", "stem", "syncbn_comm", "synthetic",
    "synthetic_size", "tb_folder", "tb_path", "val_batch_size", "val_folder", "warm", "weight_decay", "work_dir",
    "world_size",
}


def _parse(tmp_path, extra, make_dirs=False):
    return parse_linear(["--work_dir", str(tmp_path)] + extra, make_dirs=make_dirs, now=NOW)


def test_heads_are_the_product_lr_major(tmp_path):
    o = _parse(tmp_path, ["--sweep_lr", "0.5", "1", "5", "--sweep_wd", "0", "1e-3"])
    assert o.sweep == [(0.5, 0.0), (0.5, 1e-3), (1.0, 0.0), (1.0, 1e-3), (5.0, 0.0), (5.0, 1e-3)]
    assert o.model_name == "cifar10_resnet50_lr_0.1_decay_0_bsz_512_sweep6"
    assert o.save_folder.endswith("_sweep6") and o.tb_folder.endswith("_sweep6")


def test_an_absent_list_is_the_single_flag(tmp_path):
    o = _parse(tmp_path, ["--sweep_lr", "1", "2", "--weight_decay", "1e-4"])
    assert o.sweep == [(1.0, 1e-4), (2.0, 1e-4)]
    o = _parse(tmp_path, ["--sweep_wd", "0", "1e-4", "--learning_rate", "5"])
    assert o.sweep == [(5.0, 0.0), (5.0, 1e-4)]
    assert o.learning_rate == 5 and o.weight_decay == 0       # the single flags keep their values
    o = _parse(tmp_path, ["--sweep_lr", "3"])
    assert o.sweep == [(3.0, 0.0)] and o.model_name.endswith("_sweep1")


def test_suffix_follows_cosine_and_warm(tmp_path):
    o = _parse(tmp_path, ["--cosine", "--warm", "--sweep_lr", "1", "2"])
    assert o.model_name == "cifar10_resnet50_lr_0.1_decay_0_bsz_512_cosine_warm_sweep2"


def test_sixteen_heads_at_most(tmp_path):
    lrs = [str(0.1 * (i + 1)) for i in range(8)]
    assert len(_parse(tmp_path, ["--sweep_lr"] + lrs + ["--sweep_wd", "0", "1e-4"]).sweep) == 16
    with pytest.raises(SystemExit):
        _parse(tmp_path, ["--sweep_lr"] + lrs + ["0.9", "--sweep_wd", "0", "1e-4"])
    with pytest.raises(SystemExit):
        _parse(tmp_path, ["--sweep_lr"] + [str(0.1 * (i + 1)) for i in range(17)])


@pytest.mark.parametrize("extra", [["--sweep_lr", "0"], ["--sweep_lr", "1", "-0.5"], ["--sweep_lr", "nan"],
                                   ["--sweep_wd", "-1e-4"], ["--sweep_wd", "0", "nan"], ["--sweep_lr"],
                                   ["--sweep_lr", "fast"],
                                   ["--sweep_wd", "1e-4", "--learning_rate", "0"]])
def test_bad_values_are_parser_errors(tmp_path, extra):
    with pytest.raises(SystemExit):
        _parse(tmp_path, extra)


def test_without_the_flags_only_sweep_none_is_new(tmp_path):
    argv = ["--learning_rate", "5", "--cosine", "--batch_size", "256"]
    o = _parse(tmp_path, argv)
    assert o.sweep is None
    assert set(vars(o)) == PLAIN_KEYS | {"sweep"}
    assert o.model_name == "cifar10_resnet50_lr_5.0_decay_0_bsz_256_cosine"
    assert o.save_folder.endswith("classifier_1015_2105_" + o.model_name)
    w = _parse(tmp_path, argv + ["--warm"])
    assert set(vars(w)) == PLAIN_KEYS | {"sweep", "warmup_from", "warm_epochs", "warmup_to"}
    # a sweep changes nothing else either: the same namespace but for sweep and the names
    s = _parse(tmp_path, argv + ["--sweep_lr", "1", "2"])
    named = {"sweep", "model_name", "save_folder", "tb_folder"}
    assert {k: v for k, v in vars(s).items() if k not in named} == {k: v for k, v in vars(o).items() if k not in named}


@pytest.mark.parametrize("sched", [["--cosine"], ["--lr_decay_epochs", "3,5,7"], ["--warm"], ["--cosine", "--warm"]])
def test_head_schedule_is_the_plain_runs(tmp_path, sched):
    """Head g's lr at (epoch, batch) is exactly what a plain run with that base lr gets."""
    lrs, wds = [0.05, 1.0, 30.0], [0.0, 1e-3]
    common = ["--epochs", "12"] + sched
    o = _parse(tmp_path, common + ["--sweep_lr"] + [str(v) for v in lrs] + ["--sweep_wd"] + [str(v) for v in wds])
    heads = sweep_head_opts(o)
    assert len(heads) == 6 and o.learning_rate == 0.1           # the parsed options are untouched
    iters = 7
    for g, h in enumerate(heads):
        lr, wd = lrs[g // 2], wds[g % 2]
        plain = _parse(tmp_path, common + ["--learning_rate", str(lr), "--weight_decay", str(wd)])
        assert (h.learning_rate, h.weight_decay) == (lr, wd)
        assert h.model_name == o.model_name
        assert getattr(h, "warmup_to", None) == getattr(plain, "warmup_to", None)
        for epoch in range(1, 13):
            assert lr_at_epoch(h, epoch) == lr_at_epoch(plain, epoch)
            for b in range(iters):
                assert warmup_lr(h, epoch, b, iters) == warmup_lr(plain, epoch, b, iters)
    if "--warm" in sched:
        assert len({h.warmup_to for h in heads}) == 3           # per head, not the base lr's


def _record(eng):
    """Every (tag, value, step) the engine logs."""
    rec = []
    inner = eng.logger.log_value

    def log_value(tag, value, step):
        rec.append((tag, value, step))
        return inner(tag, value, step)

    eng.logger.log_value = log_value
    return rec


TAGS = ["train_loss", "train_acc1", "train_acc5", "val_loss", "val_acc1", "val_acc5"]


def run_sweep_and_singles(tmp_path, device, common, lrs, wd=None, extra=()):
    """One sweep run and one plain run per head; returns (engine, result, records, [(result, records, engine)])."""
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    wda = [] if wd is None else ["--weight_decay", str(wd)]
    so = parse_linear(common + list(extra) + wda + ["--sweep_lr"] + [str(v) for v in lrs]
                      + ["--work_dir", str(tmp_path / "sweep")], make_dirs=True)
    se = LinearEngine(so, device=device)
    srec = _record(se)
    sres = se.run()
    singles = []
    for i, lr in enumerate(lrs):
        po = parse_linear(common + list(extra) + wda + ["--learning_rate", str(lr), "--work_dir", str(tmp_path / f"s{i}")],
                          make_dirs=True)
        pe = LinearEngine(po, device=device)
        prec = _record(pe)
        singles.append((pe.run(), prec, pe))
    return se, sres, srec, singles


def check_sweep_equals_singles(se, sres, srec, singles, lrs, epochs):
    for g, (pres, prec, _) in enumerate(singles):
        for t in TAGS:
            got = [(v, s) for tag, v, s in srec if tag == f"classifier/{t}/h{g}"]
            want = [(v, s) for tag, v, s in prec if tag == f"classifier/{t}"]
            assert len(want) == epochs and got == want, (g, t, got, want)
    assert not [tag for tag, _, _ in srec if tag.startswith("classifier/") and "/h" not in tag]
    res = se.sweep_results
    assert [r["lr"] for r in res] == list(lrs) and len(res) == len(lrs)
    for r, (pres, _, _) in zip(res, singles):
        assert (r["best_acc"], r["best_acc5"]) == pres
        assert 0 <= r["best_epoch"] <= epochs
    best = max(res, key=lambda r: r["best_acc"])
    assert sres == (best["best_acc"], best["best_acc5"])


def test_torch_sweep_equals_single_runs(tmp_path, caplog):
    """--backend torch on the CPU: every head's epoch metrics and final weights are the plain run's."""
    from simclr_pytorch_distributed_amd.models.resnet import LinearClassifier
    common = ["--model", "resnet18", "--backend", "torch", "--synthetic", "--synthetic_size", "32", "--batch_size", "8",
              "--epochs", "2", "--max_steps", "2", "--print_freq", "1"]
    lrs = [0.05, 0.5, 2.0]
    with caplog.at_level("INFO"):
        se, sres, srec, singles = run_sweep_and_singles(tmp_path, torch.device("cpu"), common, lrs, wd=1e-3,
                                                        extra=["--cosine", "--warm"])
    assert se.native_sweep is None
    check_sweep_equals_singles(se, sres, srec, singles, lrs, 2)
    for g, (_, _, pe) in enumerate(singles):
        st = se.head_state(g)
        clf = LinearClassifier("resnet18", se.opt.n_cls)
        clf.load_state_dict(st)
        assert torch.equal(clf.fc.weight, pe.classifier.fc.weight) and torch.equal(clf.fc.bias, pe.classifier.fc.bias)
    assert not torch.equal(se.head_state(0)["fc.weight"], se.head_state(2)["fc.weight"])
    lines = [r.getMessage() for r in caplog.records]
    for g, r in enumerate(se.sweep_results):
        assert "head {} lr {:g} wd 0.001: best accuracy {:.2f}, accuracy5 {:.2f}".format(
            g, r["lr"], r["best_acc"], r["best_acc5"]) in lines
    assert "best accuracy: {:.2f}, accuracy5: {:.2f}".format(*sres) in lines
    assert any(l.startswith("Train: [1][1/2]") and l.endswith(" [h0 of 3]") for l in lines)
    assert any(l.startswith("Test: [0/") and l.endswith(" [h0 of 3]") for l in lines)


def test_sweep_weight_decay_product_on_the_torch_path(tmp_path):
    """lr x wd heads: the wd of a head is its optimizer's, and equal settings give equal heads."""
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    o = parse_linear(["--model", "resnet18", "--backend", "torch", "--synthetic", "--synthetic_size", "32",
                      "--batch_size", "8", "--epochs", "1", "--max_steps", "2",
                      "--sweep_lr", "0.5", "0.5", "--sweep_wd", "0", "0.1", "--work_dir", str(tmp_path)], make_dirs=True)
    e = LinearEngine(o, device=torch.device("cpu"))
    assert [(g["lr"], g["weight_decay"]) for op in e.optimizers for g in op.param_groups] == o.sweep
    e.run()
    w = [e.head_state(g)["fc.weight"] for g in range(4)]
    assert torch.equal(w[0], w[2]) and torch.equal(w[1], w[3]) and not torch.equal(w[0], w[1])
    assert [(r["lr"], r["wd"]) for r in e.sweep_results] == o.sweep
