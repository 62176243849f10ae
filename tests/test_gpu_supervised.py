"""Supervised cross-entropy trainer on the native path (engine/supervised.py, main_ce.py): one
step against fp32 torch, a short training run with checkpoint / reload / resume, fine-tuning
from a SupCon checkpoint, and the two-rank rehearsal on one GPU."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opt(tmp_path, *extra):
    from simclr_pytorch_distributed_amd.config import parse_ce
    return parse_ce(["--model", "resnet18", "--synthetic", "--synthetic_size", "64", "--batch_size", "16",
                     "--learning_rate", "0.05", "--print_freq", "2", "--save_freq", "1", "--val_batch_size", "500",
                     "--work_dir", str(tmp_path), *extra])


def test_one_step_parity(gpu, tmp_path):
    """One step from the same initialisation on fp32 torch, torch autocast-bf16 and native, the
    `evaluation` augmentation (normalize only: every backend sees the same pixels). Native loss
    and gradients of fc.weight, fc.bias and encoder.conv1.weight against fp32: relative error
    <= 1.5 x autocast's + 1e-2 (the gate of test_gpu_probe.py::test_folded_eval_encoder)."""
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    torch.manual_seed(5)
    init = SupCEResNet("resnet18", 10).state_dict()
    names = ("fc.weight", "fc.bias", "encoder.conv1.weight")
    res = {}
    for tag, extra in (("fp32", ["--backend", "torch", "--precision", "fp32"]),
                       ("autocast", ["--backend", "torch", "--precision", "bf16"]),
                       ("native", ["--backend", "native"])):
        eng = SupervisedEngine(_opt(tmp_path / tag, *extra), device=gpu)
        eng.model.load_state_dict(init)
        eng.model.train()
        eng.aug = AugConfig.evaluation(32, eng.opt.mean_t, eng.opt.std_t)
        idx = torch.arange(16, device=gpu)
        st = eng.train_step(idx, eng.train.labels[idx], 1, 0, 1)
        torch.cuda.synchronize()
        params = dict(eng.model.named_parameters())
        res[tag] = {"loss": st["loss_local"].double().reshape(1).clone(),
                    **{n: params[n].grad.detach().double().clone() for n in names}}
        assert abs(float(st["stats"][0]) / 16 - float(st["loss_local"])) < 1e-5
        if tag == "native":
            assert type(st["loss_local"]).__name__ == "Tensor" and eng.backend == "native"

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    for q in ("loss",) + names:
        e_n, e_c = rel(res["native"][q], res["fp32"][q]), rel(res["autocast"][q], res["fp32"][q])
        print(f"{q}: native rel error {e_n:.4g} (autocast {e_c:.4g})")
        assert e_n <= 1.5 * e_c + 1e-2, q


def test_train_checkpoint_resume(gpu, tmp_path):
    """Two epochs of a 64-image synthetic run on native: a checkpoint is written, reloads into
    SupCEResNet, --resume continues at epoch 3, and the native validation top-1 equals the torch
    eval-mode top-1 of the reloaded model on the same images to within one image."""
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, augment, nhwc8_to_nchw
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    opt = _opt(tmp_path, "--backend", "native", "--epochs", "2")
    eng = SupervisedEngine(opt, device=gpu)
    last = eng.run()
    assert os.path.exists(last) and os.path.exists(os.path.join(opt.save_folder, "ckpt_epoch_2.pth"))
    assert [h["epoch"] for h in eng.history] == [1, 2] and eng.global_step == 8
    assert all(h["train_loss"] == h["train_loss"] and "val_acc" in h for h in eng.history)
    st = ckpt_mod.load_checkpoint(last)
    assert set(st) == {"opt", "model", "optimizer", "epoch", "sdx_state"} and st["epoch"] == 2
    m = SupCEResNet("resnet18", 10)
    ckpt_mod.load_model_state(m, st["model"])                  # strict: every key, nothing else
    m = m.to(gpu).eval()
    n = len(eng.val)
    with torch.no_grad():
        x = augment(eng.val.images, torch.arange(n, device=gpu), AugConfig.evaluation(32, opt.mean_t, opt.std_t), 0)
        hits_t = int((m(nhwc8_to_nchw(x).float()).argmax(1) == eng.val.labels).sum())
    _, acc1, _ = eng.validate()
    hits_n = acc1 * n / 100.0
    print(f"validation top-1 hits: native {hits_n:.1f}, torch eval of the reloaded model {hits_t} (of {n})")
    assert abs(hits_n - round(hits_n)) < 1e-6 and abs(round(hits_n) - hits_t) <= 1
    assert abs(acc1 - eng.history[-1]["val_acc"]) < 1e-9
    eng2 = SupervisedEngine(_opt(tmp_path, "--backend", "native", "--epochs", "3", "--resume", last), device=gpu)
    assert eng2.start_epoch == 3 and eng2.global_step == 8
    assert torch.equal(eng2.flat.flat, eng.flat.flat)
    eng2.run()
    assert [h["epoch"] for h in eng2.history] == [3] and eng2.global_step == 12


def test_fine_tune_from_supcon_checkpoint(gpu, tmp_path):
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet, SupConResNet
    torch.manual_seed(11)
    src = SupConResNet("resnet18")
    path = str(tmp_path / "supcon.pth")
    ckpt_mod.save_model(src, torch.optim.SGD(src.parameters(), lr=0.1), {"model": "resnet18"}, 1, path)
    opt = _opt(tmp_path, "--backend", "native", "--epochs", "1", "--ckpt", path, "--label_frac", "0.5")
    eng = SupervisedEngine(opt, device=gpu)
    own = eng.model.state_dict()
    enc = src.encoder.state_dict()
    assert len(enc) > 100
    for k, v in enc.items():
        assert torch.equal(own["encoder." + k].cpu(), v), k
    torch.manual_seed(opt.seed)
    fresh = SupCEResNet("resnet18", 10)
    assert torch.equal(own["fc.weight"].cpu(), fresh.fc.weight) and torch.equal(own["fc.bias"].cpu(), fresh.fc.bias)
    eng.run()                                                   # trains on the labelled half
    assert eng.history[0]["train_loss"] == eng.history[0]["train_loss"]


def _launch(world, out):
    rdv = os.path.join(str(out), f"rdv_ce_{world}")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), SDX_CONV_CFG="4",
                   MASTER_ADDR="127.0.0.1", SDX_INIT_METHOD="file://" + rdv, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_ce_worker.py"), str(out)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        try:
            _, err = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("distributed worker timed out")
        assert p.returncode == 0, err[-3000:]


def test_two_rank_step_equals_single_rank(gpu, tmp_path):
    """W = 2 (two processes on this GPU, gloo, SyncBN, bucket reducer) against the W = 1 step on
    the concatenated batch: the gradients the optimizer applies to fc and conv1 match (ResNet-18
    bar of tests/test_gpu_dist.py: relative error < 2e-2), the replicas stay identical."""
    _launch(1, tmp_path)
    _launch(2, tmp_path)
    ref = torch.load(tmp_path / "ce_w1_r0.pt", weights_only=True)
    a = torch.load(tmp_path / "ce_w2_r0.pt", weights_only=True)
    b = torch.load(tmp_path / "ce_w2_r1.pt", weights_only=True)
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["flat"], b["flat"])
    assert "fc.weight" in a["names"] and a["names"] == ref["names"]
    for n, o, k in zip(a["names"], a["offsets"], a["numels"]):
        if n in ("fc.weight", "fc.bias", "encoder.conv1.weight"):
            g1, g2 = ref["grad"][o:o + k].double(), a["grad"][o:o + k].double()
            r = float((g2 - g1).norm() / (g1.norm() + 1e-12))
            print(f"{n}: W=2 vs W=1 gradient rel {r:.3g}")
            assert r < 2e-2, (n, r)
    # the global mean loss is the mean of the ranks' local means; the hit counts add up
    assert abs(0.5 * (a["loss"] + b["loss"]) - ref["loss"]) < 1e-2 * abs(ref["loss"]) + 1e-3
    assert abs(float((a["stats"] + b["stats"] - ref["stats"])[0])) < 1e-2 * float(ref["stats"][0]) + 1e-3
