"""Weighted k-NN evaluation on the CPU: the torch reference against a brute-force fp64
oracle, the tie rule, the flags, the evaluator's no-side-effect contract, the two-rank
sharded evaluation and the TensorBoard tags of a tiny pretraining run."""
import datetime
import math
import os
import socket
import subprocess
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from simclr_pytorch_distributed_amd.config import parse_linear, parse_pretrain
from simclr_pytorch_distributed_amd.ops.knn import hit_counts, knn_classify, knn_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


def _unit(n, d, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, d, generator=g, dtype=dtype), dim=1)


def _oracle(q, bank, bank_labels, n_cls, k, T):
    """Full sort by (-sim, idx) and a Python vote, fp64."""
    sim = (q.double() @ bank.double().t()).tolist()
    scores = torch.zeros(len(sim), n_cls, dtype=torch.float64)
    sims, idxs = [], []
    for r, row in enumerate(sim):
        order = sorted(range(len(row)), key=lambda j: (-row[j], j))[:k]
        for j in order:
            scores[r, int(bank_labels[j])] += math.exp(row[j] / T)
        sims.append([row[j] for j in order])
        idxs.append(order)
    return scores, torch.tensor(sims, dtype=torch.float64), torch.tensor(idxs)


@pytest.mark.parametrize("k", [1, 20, 257])
def test_reference_matches_bruteforce_oracle(k):
    q, bank = _unit(33, 64, 1), _unit(257, 64, 2)
    labels = torch.randint(0, 7, (257,), generator=torch.Generator().manual_seed(3))
    scores, sims, idx = knn_reference(q, bank, labels, 7, k, 0.1)
    o_scores, o_sims, o_idx = _oracle(q, bank, labels, 7, k, 0.1)
    assert scores.dtype == torch.float64 and sims.shape == (33, k)
    assert torch.equal(idx, o_idx)
    assert torch.equal(sims, o_sims)
    assert torch.allclose(scores, o_scores, rtol=1e-12, atol=0.0)


def test_three_row_bank_weights_and_tie_rule():
    # rows 0 and 2 are the same vector: the duplicate resolves to the lower index
    bank = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]], dtype=torch.float64)
    labels = torch.tensor([0, 1, 2])
    q = torch.tensor([[1.0, 0.0], [0.6, 0.8]], dtype=torch.float64)
    T = 0.5
    scores, sims, idx = knn_reference(q, bank, labels, 3, 2, T)
    assert idx.tolist() == [[0, 2], [1, 0]]
    assert torch.equal(sims, torch.tensor([[1.0, 1.0], [0.8, 0.6]], dtype=torch.float64))
    e = math.exp
    want = torch.tensor([[e(1 / T), 0.0, e(1 / T)], [e(0.6 / T), e(0.8 / T), 0.0]], dtype=torch.float64)
    assert torch.allclose(scores, want, rtol=1e-14, atol=0.0)
    _, _, idx1 = knn_reference(q, bank, labels, 3, 1, T)
    assert idx1.tolist() == [[0], [1]]
    # k larger than the bank is clamped; hits follow the rank rule #{c: score_c > score_label} < kk
    sc, st = knn_classify(q, bank, labels, 3, k=9, T=T, labels=torch.tensor([2, 1]))
    assert sc.shape == (2, 3)
    assert st.tolist() == [2.0, 2.0]       # query 0: classes 0 and 2 tie -> nothing is strictly above the label
    assert hit_counts(sc, torch.tensor([1, 0])).tolist() == [0.0, 2.0]


def test_flags_defaults_and_names_unchanged(tmp_path):
    now = datetime.datetime(2024, 1, 2, 3, 4)
    base = ["--model", "resnet18", "--synthetic", "--work_dir", str(tmp_path)]
    a = parse_pretrain(base, make_dirs=False, now=now)
    assert (a.knn_freq, a.knn_k, a.knn_t) == (0, 200, 0.1)
    b = parse_pretrain(base + ["--knn_freq", "5", "--knn_k", "20", "--knn_t", "0.07"], make_dirs=False, now=now)
    assert (b.knn_freq, b.knn_k, b.knn_t) == (5, 20, 0.07)
    for f in ("model_name", "save_folder", "tb_folder"):
        assert getattr(a, f) == getattr(b, f)
    la = parse_linear(base, make_dirs=False, now=now)
    assert (la.knn, la.knn_k, la.knn_t) == (False, 200, 0.1)
    lb = parse_linear(base + ["--knn", "--knn_k", "50", "--knn_t", "0.2"], make_dirs=False, now=now)
    assert (lb.knn, lb.knn_k, lb.knn_t) == (True, 50, 0.2)
    for f in ("model_name", "save_folder", "tb_folder"):
        assert getattr(la, f) == getattr(lb, f)
    with pytest.raises(ValueError, match="validation split"):
        parse_pretrain(["--dataset", "path", "--data_folder", str(tmp_path), "--mean", "(0.5,0.5,0.5)", "--std",
                        "(0.2,0.2,0.2)", "--knn_freq", "1", "--work_dir", str(tmp_path)], make_dirs=False, now=now)


def _synthetic(n_bank=64, n_val=32):
    from simclr_pytorch_distributed_amd.data.datasets import synthetic_dataset
    tr = synthetic_dataset(n_bank, 32, 10, 0, class_seed=0)
    va = synthetic_dataset(n_val, 32, 10, 1, class_seed=0)
    t = torch.from_numpy
    return t(tr.images), t(tr.labels), t(va.images), t(va.labels)


def _evaluator(n_bank=64, n_val=32, k=20):
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    from simclr_pytorch_distributed_amd.data.store import DeviceStore
    from simclr_pytorch_distributed_amd.engine.knn import KnnEvaluator
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    torch.manual_seed(0)
    model = SupConResNet("resnet18", "mlp", 128, "cifar")
    model.train()
    bx, by, vx, vy = _synthetic(n_bank, n_val)
    return model, KnnEvaluator(model, "torch", "fp32", DeviceStore(bx, by), DeviceStore(vx, vy),
                               AugConfig.evaluation(32, MEAN, STD), 10, k=k, T=0.1, batch_size=32)


def test_evaluator_cpu_has_no_side_effects():
    model, ev = _evaluator()
    model.encoder.layer1.eval()          # a mixed train/eval state must come back as it was
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [m.training for m in model.modules()]
    rng = torch.get_rng_state()
    top1, top5 = ev.evaluate()
    assert 0.0 <= top1 <= top5 <= 100.0
    assert torch.equal(torch.get_rng_state(), rng)
    assert [m.training for m in model.modules()] == flags and model.training
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert any("num_batches_tracked" in k for k in before) and any("running_var" in k for k in before)
    # the bank features are the L2-normalised encoder output, not the projection head's
    assert ev.last_bank.shape == (64, 512) and ev.last_bank.dtype == torch.float32
    assert torch.allclose(ev.last_bank.norm(dim=1), torch.ones(64), atol=1e-5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_entry(rank, world, port, d):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, ev = _evaluator(63, 31)
        res = ev.evaluate()
        assert ev.last_bank.shape[0] == 63
        torch.save(torch.tensor(res, dtype=torch.float64), os.path.join(d, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_equal_single_process():
    torch.set_num_threads(1)
    _, ev = _evaluator(63, 31)          # neither size divides by 2
    single = torch.tensor(ev.evaluate(), dtype=torch.float64)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank_entry, args=(2, _free_port(), d), nprocs=2, join=True)
        got = [torch.load(os.path.join(d, f"r{r}.pt")) for r in range(2)]
    assert torch.equal(got[0], single) and torch.equal(got[1], single), (single, got)


def _tiny_run(tmp_path, knn_freq, monkeypatch):
    from simclr_pytorch_distributed_amd.data import store
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    real = store.build_dataset

    def small_val(dataset, folder, train=True, synthetic=False, synthetic_size=50000, *a, **k):
        # the synthetic validation split has at least 1000 images; 32 are enough to see the tags
        ds = real(dataset, folder, train, synthetic, synthetic_size, *a, **k)
        if not train:
            ds.images, ds.labels = ds.images[:32], ds.labels[:32]
        return ds

    monkeypatch.setattr(store, "build_dataset", small_val)
    from simclr_pytorch_distributed_amd.utils.tb import read_events
    opt = parse_pretrain(["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32",
                          "--epochs", "2", "--max_steps", "1", "--backend", "torch", "--precision", "fp32",
                          "--learning_rate", "0.1", "--knn_freq", str(knn_freq), "--knn_k", "10", "--save_freq", "100",
                          "--work_dir", str(tmp_path / f"ws{knn_freq}")])
    eng = PretrainEngine(opt, device=torch.device("cpu"))
    path = eng.logger.path
    eng.run()
    return read_events(path)


def test_tiny_pretrain_run_writes_knn_tags(tmp_path, monkeypatch):
    ev = _tiny_run(tmp_path, 1, monkeypatch)
    for tag in ("knn/val_acc1", "knn/val_acc5"):
        got = [(s, v) for s, t, v in ev if t == tag]
        assert [s for s, _ in got] == [1, 2], (tag, got)
        assert all(0.0 <= v <= 100.0 for _, v in got)
    assert any(t == "loss" for _, t, _ in ev)


def test_tiny_pretrain_run_without_flag_has_no_knn_tags(tmp_path, monkeypatch):
    ev = _tiny_run(tmp_path, 0, monkeypatch)
    assert any(t == "loss" for _, t, _ in ev)
    assert not [t for _, t, _ in ev if t is not None and t.startswith("knn/")]


def test_plan_arithmetic_under_sanitizers(tmp_path):
    """The binding layer's split / workspace arithmetic (csrc/include/knn_plan.h) in a
    stand-alone program built with AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "knn_plan_check")
    src = os.path.join(ROOT, "csrc", "tools", "knn_plan_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", f"-I{os.path.join(ROOT, 'csrc', 'include')}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "KNN-PLAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
