#!/usr/bin/env python3
"""SwAV loss: the native kernels (csrc/kernels/swav.hip) against the fp32 torch twin
(losses/swav.py swav_reference) on the same GPU.

Every (N, D, K) is warmed up, then timed in interleaved rounds baseline, native, baseline: the two
baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``. Forward + backward to z1, z2 and C, then the stage ops singly
(device events around one op: launch gaps included). A row where native is slower says so.

``--step`` also times one ResNet-50 CIFAR step (256 images, synthetic data, native backend) of
``--method SimCLR``, ``--method SwAV`` and SimCLR again, in this process, ``--windows`` windows of 20
steps after 20 warm-up steps. Needs a GPU; there is no CPU fall-back.

    python tools/swav_bench.py [--rounds 7] [--iters 20] [--step] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.swav import swav_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, swav  # noqa: E402

SHAPES = [(n, 128, k) for n in (256, 1024) for k in (1000, 3000, 16384)]
EPS, TEMP, ITERS = 0.05, 0.1, 3


def bench_shape(n, d, k, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d + k)
    z1 = torch.randn(n, d, device=dev, generator=gen).requires_grad_(True)
    z2 = (0.5 * z1.detach() + torch.randn(n, d, device=dev, generator=gen)).requires_grad_(True)
    C = torch.nn.functional.normalize(torch.randn(k, d, device=dev, generator=gen), dim=1).requires_grad_(True)

    def run(fn):
        def f():
            z1.grad = z2.grad = C.grad = None
            fn(z1, z2, C, EPS, TEMP, ITERS).backward()
        return f

    twin, native = run(swav_reference), run(swav.swav_loss)
    twin()
    gz, gc = z1.grad.clone(), C.grad.clone()
    native()
    rz = ((z1.grad - gz).abs().max() / gz.abs().max()).item()
    rc = ((C.grad - gc).abs().max() / gc.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    emit(f"N={n:5d} D={d:4d} K={k:6d}  twin {a:8.3f} / {b:8.3f} ms (two series)  native {nat:8.3f} ms "
         f"[{lo:.3f} .. {hi:.3f}]  twin/native {0.5 * (a + b) / nat:5.2f}x{'  NATIVE SLOWER' if nat > min(a, b) else ''}"
         f"  dz diff/max {rz:.2e}  dC diff/max {rc:.2e}")
    a1, a2, Cd = z1.detach(), z2.detach(), C.detach().clone()
    zhat, rnorm = m.swav_prep(a1, a2, Cd)
    S, part = m.swav_scores(zhat, Cd, EPS)
    r = m.swav_rowsum(part)
    u, c = m.swav_sinkhorn(S, r, EPS, True)
    _, dS, _ = m.swav_loss_grad(S, u, c, EPS, TEMP)
    g = torch.ones(1, device=dev)
    stages = {"swav_prep": lambda: m.swav_prep(a1, a2, Cd),
              "swav_scores": lambda: m.swav_scores(zhat, Cd, EPS),
              "swav_rowsum": lambda: m.swav_rowsum(part),
              "swav_sinkhorn": lambda: m.swav_sinkhorn(S, r, EPS, False),
              "swav_sinkhorn (last)": lambda: m.swav_sinkhorn(S, r, EPS, True),
              "swav_loss_grad + finish": lambda: m.swav_loss_grad(S, u, c, EPS, TEMP),
              "swav_bwd": lambda: m.swav_bwd(zhat, rnorm, Cd, dS, g, False),
              "swav_bwd (frozen)": lambda: m.swav_bwd(zhat, rnorm, Cd, dS, g, True)}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    emit(f"    stages: {'  '.join(parts)}")


def bench_step(windows, emit):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    dev = torch.device("cuda:0")
    for method in (["--method", "SimCLR"], ["--method", "SwAV", "--swav_freeze_iters", "0"], ["--method", "SimCLR"]):
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
        raise SystemExit("swav_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"swav_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians")
    for n, d, k in SHAPES:
        bench_shape(n, d, k, a.rounds, a.iters, emit)
    if a.step:
        emit("ResNet-50 CIFAR step, 256 images (ms/step per window of 20 steps):")
        bench_step(a.windows, emit)


if __name__ == "__main__":
    main()
