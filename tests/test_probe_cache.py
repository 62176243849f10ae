"""--cache_features / --cache_views of the linear probe without a GPU: the parser, and LinearEngine on
the torch backend — validation on cached features reports exactly what re-encoding reports, a run on
the training bank leaves exactly the weights of a hand loop over bank[rows] in the sampler's order,
the encoder runs once per extracted batch and never again, and a bank that does not fit is refused
before anything is encoded. tests/test_gpu_probe_cache.py runs the same checks on the native path."""
import dataclasses
import datetime

import pytest
import torch

from simclr_pytorch_distributed_amd.config import parse_linear
from simclr_pytorch_distributed_amd.optim.schedules import (adjust_learning_rate, lr_at_epoch, warmup_learning_rate,
                                                            warmup_lr)

NOW = datetime.datetime(2026, 10, 21, 9, 30)
N_TRAIN, N_VAL, BATCH, VAL_BATCH, EPOCHS = 96, 40, 40, 16, 2
TRAIN_BATCHES, VAL_BATCHES = 3, 3            # ceil(96 / 40), ceil(40 / 16): the last batch of each is partial
SWEEP_LRS = ["0.5", "1", "2"]


def _parse(tmp_path, extra):
    return parse_linear(["--work_dir", str(tmp_path)] + extra, make_dirs=False, now=NOW)


def test_parser_accepts_the_modes(tmp_path):
    o = _parse(tmp_path, [])
    assert (o.cache_features, o.cache_views) == ("off", 0)
    assert "cache_features" not in vars(o) and "cache_views" not in vars(o)      # an absent flag adds no option
    assert _parse(tmp_path, ["--cache_features", "off"]).cache_features == "off"
    o = _parse(tmp_path, ["--cache_features", "val"])
    assert (o.cache_features, o.cache_views) == ("val", 0)
    o = _parse(tmp_path, ["--cache_features", "all"])
    assert (o.cache_features, o.cache_views) == ("all", 0)
    o = _parse(tmp_path, ["--cache_features", "all", "--cache_views", "4", "--sweep_lr", "1", "2", "--head_gemm", "mfma",
                          "--knn", "--max_steps", "3"])
    assert (o.cache_features, o.cache_views, len(o.sweep), o.head_gemm) == ("all", 4, 2, "mfma")
    assert _parse(tmp_path, ["--cache_features", "val", "--cache_views", "0"]).cache_views == 0


@pytest.mark.parametrize("extra,reason", [
    (["--cache_views", "2"], "--cache_views 2 needs --cache_features all (got off)"),
    (["--cache_features", "val", "--cache_views", "1"], "--cache_views 1 needs --cache_features all (got val)"),
    (["--cache_features", "off", "--cache_views", "3"], "--cache_views 3 needs --cache_features all (got off)"),
    (["--cache_features", "all", "--cache_views", "-1"], "--cache_views -1: the number of cached views cannot be negative"),
    (["--cache_views", "-1"], "--cache_views -1: the number of cached views cannot be negative"),
    (["--cache_features", "train"], "argument --cache_features: invalid choice: 'train'"),
    (["--cache_features"], "argument --cache_features: expected one argument"),
    (["--cache_features", "all", "--cache_views", "two"], "argument --cache_views: invalid int value: 'two'")])
def test_parser_rejects(tmp_path, extra, reason, capsys):
    """Every rejected combination exits with its own reason on stderr."""
    with pytest.raises(SystemExit):
        _parse(tmp_path, extra)
    assert reason in capsys.readouterr().err


def make_engine(tmp_path, device, backend, tag, cache=None, views=None, sweep=False, head_gemm=None, extra=()):
    """A ResNet-18 probe of 96 training and 40 validation images (batches of 40 and 16, 2 epochs);
    ``eng.encoder_calls`` counts the encoder passes, ``eng.val_results`` collects validate()'s returns."""
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    argv = ["--model", "resnet18", "--backend", backend, "--synthetic", "--synthetic_size", str(N_TRAIN),
            "--batch_size", str(BATCH), "--val_batch_size", str(VAL_BATCH), "--epochs", str(EPOCHS), "--print_freq", "2",
            "--learning_rate", "0.5", "--weight_decay", "1e-3", "--warm", "--cosine",
            "--work_dir", str(tmp_path / tag)] + list(extra)
    if sweep:
        argv += ["--sweep_lr"] + SWEEP_LRS
    if head_gemm:
        argv += ["--head_gemm", head_gemm]
    if cache:
        argv += ["--cache_features", cache]
    if views is not None:
        argv += ["--cache_views", str(views)]
    eng = LinearEngine(parse_linear(argv, make_dirs=True), device=device)
    assert len(eng.train) == N_TRAIN
    eng.val = dataclasses.replace(eng.val, images=eng.val.images[:N_VAL], labels=eng.val.labels[:N_VAL])
    eng.encoder_calls = 0
    encode = eng.raw_encode = eng.encode

    def counted(x):
        eng.encoder_calls += 1
        return encode(x)

    eng.encode = counted
    eng.val_results = []
    validate = eng.validate

    def recorded():
        r = validate()
        eng.val_results.append(r)
        return r

    eng.validate = recorded
    return eng


def weights(eng):
    """[(W, b)] of every head."""
    if eng.sweep:
        return [(st["fc.weight"], st["fc.bias"]) for st in (eng.head_state(g) for g in range(len(eng.sweep)))]
    return [(eng.classifier.fc.weight.detach(), eng.classifier.fc.bias.detach())]


def hand_loop(ref, bank):
    """Train ``ref``'s classifier(s) with the ops an uncached run uses, on bank[rows] in the sampler's order."""
    opt = ref.opt
    for epoch in range(1, opt.epochs + 1):
        if ref.sweep:
            ref._set_head_lrs([lr_at_epoch(o, epoch) for o in ref.head_opts])
        else:
            adjust_learning_rate(opt, ref.optimizer, epoch)
        ref.sampler.set_epoch(epoch)
        iters = len(ref.sampler)
        for i, idx in enumerate(ref.sampler.batches(ref.device)):
            rows = bank.rows_for(idx, epoch)
            feats, labels = bank.feats[rows].contiguous(), bank.labels[rows]
            if ref.sweep:
                ref._set_head_lrs([warmup_lr(o, epoch, i, iters) for o in ref.head_opts])
                ref._classify_sweep(feats, labels, True)
            else:
                warmup_learning_rate(opt, epoch, i, iters, ref.optimizer)
                ref._classify(feats, labels, True)


def check_bank_content(eng):
    """The banks against encodes made here, batch by batch as the extraction pass is documented:
    the validation bank and a V = 0 training bank under the evaluation transform (seed 0), view v of
    batch i of a V >= 1 bank under AugConfig.linear_train with step_seed(seed, v + 1, i, 0)."""
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    from simclr_pytorch_distributed_amd.engine.base import step_seed
    opt, dev = eng.opt, eng.device

    def fresh(store, cfg, batch, v, seeded):
        out = []
        for i, s in enumerate(range(0, len(store), batch)):
            idx = torch.arange(s, min(s + batch, len(store)), device=dev)
            out.append(eng.raw_encode(store.views(idx, cfg, step_seed(opt.seed, v + 1, i, 0) if seeded else 0)).float())
        return torch.cat(out)

    assert torch.equal(eng.val_bank.feats, fresh(eng.val, eng.aug_val, VAL_BATCH, 0, False))
    assert torch.equal(eng.val_bank.labels, eng.val.labels.long())
    if eng.bank is None:
        return
    if eng.cache_views == 0:
        assert torch.equal(eng.bank.feats, fresh(eng.train, eng.aug_val, BATCH, 0, False))
        return
    train_cfg = AugConfig.linear_train(opt.size, opt.mean_t, opt.std_t)
    assert train_cfg == eng.aug_train
    for v in range(eng.cache_views):
        want = fresh(eng.train, train_cfg, BATCH, v, True)
        assert torch.equal(eng.bank.feats[v * N_TRAIN:(v + 1) * N_TRAIN], want)
        assert not torch.equal(want, fresh(eng.train, eng.aug_val, BATCH, 0, False))      # augmented, not the evaluation view


def check_val_equals_off(tmp_path, device, backend, sweep, head_gemm=None):
    off = make_engine(tmp_path, device, backend, "off", None, None, sweep, head_gemm)
    res_off = off.run()
    val = make_engine(tmp_path, device, backend, "val", "val", None, sweep, head_gemm)
    res_val = val.run()
    assert val.val_bank is not None and val.bank is None and off.val_bank is None
    assert val.val_bank.feats.shape == (N_VAL, 512) and val.val_bank.feats.dtype == torch.float32
    assert len(off.val_results) == EPOCHS and val.val_results == off.val_results      # (loss, acc1, acc5) per epoch
    assert res_val == res_off
    for (w0, b0), (w1, b1) in zip(weights(off), weights(val)):
        assert torch.equal(w0, w1) and torch.equal(b0, b1)
    assert off.encoder_calls == EPOCHS * (TRAIN_BATCHES + VAL_BATCHES)
    assert val.encoder_calls == VAL_BATCHES + EPOCHS * TRAIN_BATCHES
    if sweep:
        assert val.sweep_results == off.sweep_results
    check_bank_content(val)
    return off, val


def check_all_equals_hand_loop(tmp_path, device, backend, sweep, views, head_gemm=None):
    eng = make_engine(tmp_path, device, backend, f"all{views}", "all", views, sweep, head_gemm)
    eng.run()
    v = max(views, 1)
    assert eng.encoder_calls == TRAIN_BATCHES * v + VAL_BATCHES
    bank = eng.bank
    assert bank.feats.shape == (v * N_TRAIN, 512) and bank.labels.shape == (v * N_TRAIN,)
    assert torch.equal(bank.labels, eng.train.labels.long().repeat(v))
    idx = torch.tensor([5, 0, N_TRAIN - 1], device=bank.feats.device)
    assert torch.equal(bank.rows_for(idx, 1), idx)
    if views == 2:
        # epoch 1 trains on view 0, epoch 2 on view 1, epoch 3 on view 0 again; the views are different draws
        assert torch.equal(bank.rows_for(idx, 2), idx + N_TRAIN) and torch.equal(bank.rows_for(idx, 3), idx)
        assert not torch.equal(bank.feats[:N_TRAIN], bank.feats[N_TRAIN:])
        for e in (1, 2):
            f, y = bank.epoch_view(e)
            assert torch.equal(f, bank.feats[bank.rows_for(torch.arange(N_TRAIN, device=f.device), e)])
            assert torch.equal(y, eng.train.labels.long())
    check_bank_content(eng)
    ref = make_engine(tmp_path, device, backend, f"ref{views}", None, None, sweep, head_gemm)
    start = [(w.clone(), b.clone()) for w, b in weights(ref)]
    hand_loop(ref, bank)
    assert ref.encoder_calls == 0
    for (w0, b0), (w1, b1), (ws, _) in zip(weights(ref), weights(eng), start):
        assert torch.equal(w0, w1) and torch.equal(b0, b1)
        assert not torch.equal(w0, ws)
    return eng


@pytest.mark.parametrize("sweep", [False, True], ids=["single", "sweep"])
def test_val_cache_equals_off_on_the_torch_path(tmp_path, sweep):
    off, val = check_val_equals_off(tmp_path, torch.device("cpu"), "torch", sweep)
    assert val.native_ce is None and val.native_sweep is None


@pytest.mark.parametrize("sweep,views", [(False, 0), (False, 2), (True, 2)], ids=["single-V0", "single-V2", "sweep-V2"])
def test_bank_training_equals_hand_loop_on_the_torch_path(tmp_path, caplog, sweep, views):
    with caplog.at_level("INFO"):
        eng = check_all_equals_hand_loop(tmp_path, torch.device("cpu"), "torch", sweep, views)
    rows = max(views, 1) * N_TRAIN
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("feature cache")]
    assert len(lines) == 1                                                        # one line: shapes and bytes
    assert f"val bank [{N_VAL}, 512]" in lines[0] and f"train bank [{rows}, 512]" in lines[0]
    assert f"{(N_VAL + rows) * (512 * 4 + 8)} bytes" in lines[0]
    assert any(m.getMessage().startswith("best accuracy:") for m in caplog.records)


def test_a_bank_that_does_not_fit_is_refused_before_encoding(tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine import linear
    need = (N_VAL + 2 * N_TRAIN) * (512 * 4 + 8)
    eng = make_engine(tmp_path, torch.device("cpu"), "torch", "oom", "all", 2)
    monkeypatch.setattr(linear, "free_memory", lambda device: need - 1)
    with pytest.raises(RuntimeError, match=rf"need {need} bytes.*{need - 1} free"):
        eng.run()
    assert eng.encoder_calls == 0 and eng.bank is None and eng.val_bank is None
    monkeypatch.setattr(linear, "free_memory", lambda device: need)               # exactly enough: accepted
    eng.prepare_cache()
    assert eng.encoder_calls == 2 * TRAIN_BATCHES + VAL_BATCHES


def test_refusal_names_what_the_mode_can_drop(tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine import linear
    monkeypatch.setattr(linear, "free_memory", lambda device: 0)
    val = make_engine(tmp_path, torch.device("cpu"), "torch", "oomval", "val")
    with pytest.raises(RuntimeError) as e:
        val.prepare_cache()
    assert str(e.value).endswith("use --cache_features off") and "cache_views" not in str(e.value)
    assert f"val [{N_VAL}, 512]" in str(e.value) and "train" not in str(e.value)
    al = make_engine(tmp_path, torch.device("cpu"), "torch", "oomall", "all", 0)
    with pytest.raises(RuntimeError, match="use --cache_features val, fewer --cache_views or a smaller dataset"):
        al.prepare_cache()
    assert val.encoder_calls == 0 and al.encoder_calls == 0


def test_free_memory_is_unknown_without_a_gpu():
    from simclr_pytorch_distributed_amd.engine.linear import free_memory
    assert free_memory(torch.device("cpu")) is None


def test_max_steps_and_profile_phases(tmp_path, caplog):
    """--max_steps bounds the classifier steps, not the extraction; under --profile the epochs time
    gather / classifier and only the extraction pass times augment / encoder."""
    eng = make_engine(tmp_path, torch.device("cpu"), "torch", "steps", "all", 0, extra=["--max_steps", "2", "--profile"])
    with caplog.at_level("INFO"):
        eng.run()
    assert eng.encoder_calls == TRAIN_BATCHES + VAL_BATCHES
    phases = [r.getMessage() for r in caplog.records if r.getMessage().startswith("phases")]
    assert phases[0].startswith("phases (ms/batch, extraction): augment ") and " encoder " in phases[0]
    assert len(phases) > 1
    for line in phases[1:]:
        assert "gather" in line and "classifier" in line and "encoder" not in line and "augment" not in line
