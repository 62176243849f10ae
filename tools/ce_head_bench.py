#!/usr/bin/env python3
"""Time of the trainable classifier + cross-entropy node next to fp32 torch, and of one
supervised step next to the SimCLR step.

  kernels  forward + backward of ops/ce_head.py classifier_ce (two launches) at B x K for each C,
           against F.linear + F.cross_entropy forward + backward in fp32 torch on the same
           tensors. Interleaved rounds in one process, device events around a burst of
           iterations, median and range over the rounds.
  step     one supervised step (SupervisedEngine, ResNet-50 CIFAR stem, bf16, --images per step)
           and one SimCLR step of PretrainEngine on the same number of images (twice the encoder
           rows: two views), same interleaving.

  python tools/ce_head_bench.py kernels [--batch 512] [--feat 2048] [--classes 10 100 1000]
  python tools/ce_head_bench.py step [--images 256] [--model resnet50]
"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def timed(variants, rounds, iters):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def kernels(a):
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
    dev = torch.device("cuda:0")
    B, K = a.batch, a.feat
    print(f"classifier + mean cross-entropy, forward + backward, fp32, B = {B}, K = {K}; {a.rounds} interleaved "
          f"rounds x {a.iters} iterations; times in microseconds (median, min, max)")
    print(f"{'C':>5s} {'native 2 launches':>26s} {'torch fp32':>26s} {'torch / native':>15s}")
    for C in a.classes:
        torch.manual_seed(C)
        fc = torch.nn.Linear(K, C).to(dev)
        x = torch.randn(B, K, device=dev).relu().requires_grad_(True)
        y = torch.randint(0, C, (B,), device=dev)
        one = torch.ones((), device=dev)

        def native():
            loss, _ = classifier_ce(x, fc, y)
            loss.backward(one)

        def stock():
            loss = F.cross_entropy(F.linear(x, fc.weight, fc.bias), y)
            loss.backward(one)

        def clear():
            x.grad = None
            fc.weight.grad.zero_()
            fc.bias.grad.zero_()

        native()
        gn = (x.grad.clone(), fc.weight.grad.clone(), fc.bias.grad.clone())
        clear()
        stock()
        for g, h in zip(gn, (x.grad, fc.weight.grad, fc.bias.grad)):
            assert torch.allclose(g, h, rtol=1e-3, atol=1e-6), "native and torch gradients disagree"
        r = timed([("native", native), ("torch", stock)], a.rounds, a.iters)
        n, t = r["native"], r["torch"]
        print(f"{C:5d} {1e3 * n[0]:10.1f} ({1e3 * n[1]:6.1f}-{1e3 * n[2]:6.1f}) {1e3 * t[0]:10.1f} "
              f"({1e3 * t[1]:6.1f}-{1e3 * t[2]:6.1f}) {t[0] / n[0]:14.2f}x", flush=True)


def step(a):
    from simclr_pytorch_distributed_amd.config import parse_ce, parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="ce_step_")
    common = ["--model", a.model, "--backend", "native", "--synthetic", "--synthetic_size", str(4 * a.images),
              "--batch_size", str(a.images), "--work_dir", work]
    sup = SupervisedEngine(parse_ce(common, make_dirs=True), device=dev)
    sim = PretrainEngine(parse_pretrain(common + ["--method", "SimCLR"], make_dirs=True), device=dev)
    sup.model.train()
    sim.model.train()
    idx = torch.arange(a.images, device=dev)
    labels = sup.train.labels[idx]
    variants = [(f"supervised CE step, {a.images} images", lambda: sup.train_step(idx, labels, 1, 0, 10)),
                (f"SimCLR step, {2 * a.images} views", lambda: sim.train_step(idx, 1, 0, 10))]
    r = timed(variants, a.rounds, a.iters)
    print(f"one training step, {a.model} CIFAR stem, bf16, eager; {a.rounds} interleaved rounds x {a.iters} steps; "
          "milliseconds (median, min, max)")
    for name, _ in variants:
        m = r[name]
        print(f"{name:40s} {m[0]:8.3f} ({m[1]:.3f}-{m[2]:.3f})", flush=True)
    names = [n for n, _ in variants]
    print(f"supervised / SimCLR = {r[names[0]][0] / r[names[1]][0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--batch", type=int, default=512)
    k.add_argument("--feat", type=int, default=2048)
    k.add_argument("--classes", type=int, nargs="+", default=[10, 100, 1000])
    k.add_argument("--rounds", type=int, default=9)
    k.add_argument("--iters", type=int, default=50)
    s = sub.add_parser("step")
    s.add_argument("--images", type=int, default=256)
    s.add_argument("--model", default="resnet50")
    s.add_argument("--rounds", type=int, default=7)
    s.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    {"kernels": kernels, "step": step}[a.what](a)


if __name__ == "__main__":
    main()
