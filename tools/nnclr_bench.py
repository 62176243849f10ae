#!/usr/bin/env python3
"""NNCLR loss: the native kernels (csrc/kernels/nnclr.hip) against the fp32 torch twin
(losses/nnclr.py nnclr_reference) on the same GPU, and ``nnclr_search`` alone against the kernel it
stands in for, ``ops.knn.knn_topk(ẑ, queue_value, 1)``.

Every (N, D, K) is warmed up, then timed in interleaved rounds baseline, native, baseline: the two
baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``. Forward + backward to p, then the search pair, then the stage ops
singly (device events around one op: launch gaps included). A row where native is slower says so.

``--step`` also times one ResNet-50 CIFAR step (256 images, synthetic data, native backend) of
``--method SimCLR``, ``--method NNCLR`` and SimCLR again, in this process, ``--windows`` windows of 20
steps after 20 warm-up steps. Needs a GPU; there is no CPU fall-back.

    python tools/nnclr_bench.py [--rounds 7] [--iters 20] [--step] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.moco import queue_value  # noqa: E402
from simclr_pytorch_distributed_amd.losses.nnclr import nnclr_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, knn, moco, nnclr  # noqa: E402

SHAPES = [(n, 256, k) for n in (256, 1024) for k in (4096, 16384, 98304)]
TEMP = 0.1


def slower(nat, a, b):
    return "  NATIVE SLOWER" if nat > min(a, b) else ""


def bench_shape(n, d, k, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d + k)
    z = torch.randn(2 * n, d, device=dev, generator=gen)
    p = (0.5 * z + torch.randn(2 * n, d, device=dev, generator=gen)).requires_grad_(True)
    queue = moco.split_planes(torch.nn.functional.normalize(torch.randn(k, d, device=dev, generator=gen), dim=1))

    def run(fn):
        def f():
            p.grad = None
            fn(z, p, queue, TEMP).backward()
        return f

    twin, native = run(nnclr_reference), run(nnclr.nnclr_loss)
    twin()
    gp = p.grad.clone()
    native()
    rp = ((p.grad - gp).abs().max() / gp.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    s = m.nnclr_splits(n, n, d, k)
    emit(f"N={n:5d} D={d:4d} K={k:6d} splits {s[0]:3d}/{s[2]}/{s[3]}  twin {a:8.3f} / {b:8.3f} ms (two series)  "
         f"native {nat:8.3f} ms [{lo:.3f} .. {hi:.3f}]  twin/native {0.5 * (a + b) / nat:5.2f}x{slower(nat, a, b)}"
         f"  dp diff/max {rp:.2e}")
    zhat, zpl, ppl, rn = m.nnclr_prep(z, p.detach())
    bank = queue_value(queue).contiguous()
    i_knn = knn.knn_topk(zhat, bank, 1)[1][:, 0]
    idx, _, nnpl = m.nnclr_search(zpl, queue)
    a, b, nat, lo, hi = interleaved(lambda: knn.knn_topk(zhat, bank, 1), lambda: m.nnclr_search(zpl, queue), rounds,
                                    iters)
    emit(f"    search: knn_topk(k=1) {a:8.3f} / {b:8.3f} ms (two series)  nnclr_search {nat:8.3f} ms "
         f"[{lo:.3f} .. {hi:.3f}]  {0.5 * (a + b) / nat:5.2f}x{slower(nat, a, b)}  rows that differ "
         f"{(i_knn != idx).sum().item()} of {2 * n}")
    loss, lse, _ = m.nnclr_sweep_fwd(nnpl, ppl, TEMP, 0)
    g = torch.ones(1, device=dev)
    pd = p.detach()
    stages = {"nnclr_prep": lambda: m.nnclr_prep(z, pd),
              "nnclr_search (search + pick)": lambda: m.nnclr_search(zpl, queue),
              "nnclr_sweep_fwd (sweep + finish + total)": lambda: m.nnclr_sweep_fwd(nnpl, ppl, TEMP, 0),
              "nnclr_bwd (sweep + dp)": lambda: m.nnclr_bwd(nnpl, ppl, pd, rn, lse, g, TEMP, 0)}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    emit(f"    stages: {'  '.join(parts)}")


def bench_step(windows, emit):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    dev = torch.device("cuda:0")
    for method in (["--method", "SimCLR"], ["--method", "NNCLR"], ["--method", "SimCLR"]):
        with tempfile.TemporaryDirectory() as tmp:
            opt = parse_pretrain(method + ["--model", "resnet50", "--synthetic", "--synthetic_size", "2048",
                                           "--batch_size", "256", "--backend", "native", "--work_dir", tmp],
                                 make_dirs=False)
            eng = PretrainEngine(opt)
            idx = [torch.arange(256 * i, 256 * i + 256, device=dev) for i in range(8)]
            step = [0]

            def one():
                eng.train_step(idx[step[0] % 8], 1, step[0], 10 ** 6)
                step[0] += 1

            for _ in range(20):
                one()
            emit(f"     {' '.join(method):40s} " + " ".join(f"{timed(one, 20):.3f}" for _ in range(windows)))
            del eng
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nnclr_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"nnclr_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians")
    for n, d, k in SHAPES:
        bench_shape(n, d, k, a.rounds, a.iters, emit)
    if a.step:
        emit("ResNet-50 CIFAR step, 256 images (ms/step per window of 20 steps):")
        bench_step(a.windows, emit)


if __name__ == "__main__":
    main()
