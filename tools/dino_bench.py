#!/usr/bin/env python3
"""DINO loss: the native kernels (csrc/kernels/dino.hip) against the fp32 torch twin (losses/dino.py
dino_reference) on the same GPU, forward + backward to z and V.

Every (N per view, D, K) is warmed up, then timed in interleaved rounds baseline, native, baseline: the
two baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``. Then the stage ops singly (device events around one op: launch gaps
included). A row where native is slower is marked ``**...**``.

``--step`` also times one ResNet-50 CIFAR step (256 images, synthetic data, native backend) of
``--method SimCLR``, ``--method DINO`` (K = 65536, --feat_dim 256) and SimCLR again, in this process,
``--windows`` windows of 20 steps after 20 warm-up steps. Needs a GPU; there is no CPU fall-back.

    python tools/dino_bench.py [--rounds 7] [--iters 10] [--step] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.dino import dino_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, dino  # noqa: E402

SHAPES = [(n, 256, k) for n in (256, 1024) for k in (4096, 16384, 65536)]
TEMPS = (0.1, 0.04)


def bench_shape(n, d, k, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d + k)
    zs = torch.randn(2 * n, d, device=dev, generator=gen).requires_grad_(True)
    zt = 0.5 * zs.detach() + torch.randn(2 * n, d, device=dev, generator=gen)
    vs = torch.randn(k, d, device=dev, generator=gen).requires_grad_(True)
    vt = vs.detach() + 0.05 * torch.randn(k, d, device=dev, generator=gen)
    center = 0.1 * torch.randn(k, device=dev, generator=gen)

    def run(fn):
        def f():
            zs.grad, vs.grad = None, None
            fn(zs, zt, vs, vt, center, *TEMPS).backward()
        return f

    twin = run(dino_reference)
    native = run(lambda *a: dino.dino_loss(*a)[0])
    twin()
    gz, gv = zs.grad.clone(), vs.grad.clone()
    native()
    rz = ((zs.grad - gz).abs().max() / gz.abs().max()).item()
    rv = ((vs.grad - gv).abs().max() / gv.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    ks, rs = m.dino_splits(n, d, k)
    row = (f"N={n:5d} D={d:4d} K={k:6d} splits {ks:3d}/{rs:2d}  twin {a:8.3f} / {b:8.3f} ms (two series)  "
           f"native {nat:8.3f} ms [{lo:.3f} .. {hi:.3f}]  twin/native {0.5 * (a + b) / nat:5.2f}x  "
           f"dz diff/max {rz:.2e}  dV diff/max {rv:.2e}")
    emit(f"**{row}  NATIVE SLOWER**" if nat > min(a, b) else row)
    zd, vd = zs.detach(), vs.detach()
    out = m.dino_fwd(zd, zt, vd, vt, center, *TEMPS, 0)
    lse_s, lse_t, planes, rzs, rvs, zsum = out[1], out[2], out[3:7], out[7], out[8], out[9]
    g = torch.ones(1, device=dev)
    stages = {"dino_prep": lambda: m.dino_prep(zd, zt, vd, vt),
              "dino_sweep_fwd (sweep + finish)": lambda: m.dino_sweep_fwd(*planes, center, n, *TEMPS, 0),
              "dino_bwd, z only": lambda: m.dino_bwd(zd, vd, *planes, rzs, rvs, center, lse_s, lse_t, g, *TEMPS, 0, False),
              "dino_bwd, z and V": lambda: m.dino_bwd(zd, vd, *planes, rzs, rvs, center, lse_s, lse_t, g, *TEMPS, 0, True),
              "dino_center": lambda: m.dino_center(vt, zsum, center, 0.9, 2 * n)}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    emit(f"    stages: {'  '.join(parts)}")


def bench_step(windows, emit):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    dev = torch.device("cuda:0")
    for method in (["--method", "SimCLR"], ["--method", "DINO", "--feat_dim", "256"], ["--method", "SimCLR"]):
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dino_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"dino_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians; "
         f"temperatures {TEMPS}")
    for n, d, k in SHAPES:
        bench_shape(n, d, k, a.rounds, a.iters, emit)
    if a.step:
        emit("ResNet-50 CIFAR step, 256 images (ms/step per window of 20 steps):")
        bench_step(a.windows, emit)


if __name__ == "__main__":
    main()
