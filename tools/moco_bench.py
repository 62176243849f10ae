#!/usr/bin/env python3
"""MoCo loss: the native kernels (csrc/kernels/moco.hip) against the fp32 torch twin
(losses/moco.py moco_reference) on the same GPU, and the momentum encoder's ``ema_update`` against
``torch._foreach_lerp_`` over the ResNet-50 parameters.

Every (N, D, K) is warmed up, then timed in interleaved rounds baseline, native, baseline: the two
baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``. Forward + backward to q, then the stage ops singly (device events
around one op: launch gaps included). A row where native is slower says so.

``--step`` also times one ResNet-50 CIFAR step (256 images, synthetic data, native backend) of
``--method SimCLR``, ``--method MoCo`` and SimCLR again, in this process, ``--windows`` windows of 20
steps after 20 warm-up steps. Needs a GPU; there is no CPU fall-back.

    python tools/moco_bench.py [--rounds 7] [--iters 20] [--step] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.moco import moco_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, moco  # noqa: E402

SHAPES = [(n, 128, k) for n in (256, 1024) for k in (4096, 16384, 65536)]
TEMP = 0.2


def bench_shape(n, d, k, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d + k)
    q = torch.randn(n, d, device=dev, generator=gen).requires_grad_(True)
    kk = 0.5 * q.detach() + torch.randn(n, d, device=dev, generator=gen)
    queue = moco.split_planes(torch.nn.functional.normalize(torch.randn(k, d, device=dev, generator=gen), dim=1))

    def run(fn):
        def f():
            q.grad = None
            fn(q, kk, queue, TEMP).backward()
        return f

    twin, native = run(moco_reference), run(moco.moco_loss)
    twin()
    gq = q.grad.clone()
    native()
    rq = ((q.grad - gq).abs().max() / gq.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    emit(f"N={n:5d} D={d:4d} K={k:6d} splits {m.moco_splits(n, d, k):3d}  twin {a:8.3f} / {b:8.3f} ms (two series)  "
         f"native {nat:8.3f} ms [{lo:.3f} .. {hi:.3f}]  twin/native {0.5 * (a + b) / nat:5.2f}x"
         f"{'  NATIVE SLOWER' if nat > min(a, b) else ''}  dq diff/max {rq:.2e}")
    qd = q.detach()
    loss, lse, lpos, qhat, rn, khat = m.moco_fwd(qd, kk, queue, TEMP, 0)
    g = torch.ones(1, device=dev)
    ptr = torch.zeros(1, dtype=torch.int64, device=dev)
    stages = {"moco_prep": lambda: m.moco_prep(qd, kk),
              "moco_scores (sweep + finish)": lambda: m.moco_scores(qhat, lpos, queue, TEMP, 0),
              "moco_bwd (sweep + dq)": lambda: m.moco_bwd(qhat, rn, khat, queue, lse, lpos, g, TEMP, 0),
              "moco_enqueue": lambda: m.moco_enqueue(queue, ptr, khat)}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    emit(f"    stages: {'  '.join(parts)}")


def bench_ema(rounds, iters, emit):
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    dev = torch.device("cuda:0")
    fq, fk = (FlatParams(SupConResNet("resnet50").to(dev)) for _ in range(2))
    pk = [p.detach() for p in fk.params]
    pq = [p.detach() for p in fq.params]
    a, b, nat, lo, hi = interleaved(lambda: torch._foreach_lerp_(pk, pq, 1 - 0.999),
                                    lambda: moco.ema_update(fk.flat, fq.flat, 0.999), rounds, iters)
    emit(f"ema_update, ResNet-50 flat buffer ({fq.total} floats, {len(pk)} tensors): _foreach_lerp_ {a:.3f} / {b:.3f} ms "
         f"(two series)  native {nat:.3f} ms [{lo:.3f} .. {hi:.3f}]  {0.5 * (a + b) / nat:5.2f}x"
         f"{'  NATIVE SLOWER' if nat > min(a, b) else ''}")


def bench_step(windows, emit):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    dev = torch.device("cuda:0")
    for method in (["--method", "SimCLR"], ["--method", "MoCo"], ["--method", "SimCLR"]):
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
        raise SystemExit("moco_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"moco_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians")
    for n, d, k in SHAPES:
        bench_shape(n, d, k, a.rounds, a.iters, emit)
    bench_ema(a.rounds, a.iters, emit)
    if a.step:
        emit("ResNet-50 CIFAR step, 256 images (ms/step per window of 20 steps):")
        bench_step(a.windows, emit)


if __name__ == "__main__":
    main()
