#!/usr/bin/env python3
"""Barlow Twins loss, forward + backward: the native kernels (csrc/kernels/barlow.hip) against the
fp32 torch twin (losses/barlow.py barlow_reference) on the same GPU.

Every (N, D) is warmed up, then timed in interleaved rounds twin, native, twin: the two twin series
give the baseline's own spread. A round is ``--iters`` calls between two device events. The stage
ops are then timed singly the same way (device events around one op: launch gaps included, so the
stages add up to a little more than the whole). Needs a GPU; there is no CPU fall-back.

    python tools/barlow_bench.py [--rounds 7] [--iters 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.barlow import barlow_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, barlow  # noqa: E402

SHAPES = [(n, d) for n in (256, 1024) for d in (128, 2048, 8192)]
LAM, EPS = 0.0051, 1e-5


def fwd_bwd(loss_fn, z1, z2):
    def run():
        z1.grad = z2.grad = None
        loss_fn(z1, z2, LAM, EPS).backward()
    return run


def bench_shape(n, d, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d)
    z1 = torch.randn(n, d, device=dev, generator=gen).requires_grad_(True)
    z2 = (0.5 * z1.detach() + torch.randn(n, d, device=dev, generator=gen)).requires_grad_(True)
    twin, native = fwd_bwd(barlow_reference, z1, z2), fwd_bwd(barlow.barlow_loss, z1, z2)
    # same inputs, same result (fp32 twin: tolerance of its own GEMMs)
    twin()
    gt = z1.grad.clone()
    native()
    rel = ((z1.grad - gt).abs().max() / gt.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    base = 0.5 * (a + b)
    slower = nat > min(a, b)
    emit(f"N={n:5d} D={d:5d}  twin {a:8.3f} / {b:8.3f} ms (two series)  native {nat:8.3f} ms "
         f"[{lo:.3f} .. {hi:.3f}]  twin/native {base / nat:5.2f}x{'  NATIVE SLOWER' if slower else ''}"
         f"  grad diff/max {rel:.2e}")
    # stages, one op each
    a1, a2 = z1.detach(), z2.detach()
    stats = m.barlow_colstats(a1, a2, EPS)[1]
    C = m.barlow_xcorr(a1, a2, stats)
    C0 = C.clone()
    _, G, r = m.barlow_loss_grad(C0.clone(), LAM, n)
    g = torch.ones(1, device=dev)
    stages = {"bt_colstats": lambda: m.barlow_colstats(a1, a2, EPS),
              "bt_xcorr": lambda: m.barlow_xcorr(a1, a2, stats),
              "copy of C": lambda: C.copy_(C0),     # the in-place stage needs a fresh C per call:
              "copy + bt_loss_grad + finish": lambda: m.barlow_loss_grad(C.copy_(C0), LAM, n),   # subtract the copy
              "bt_bwd": lambda: m.barlow_bwd(a1, a2, G, stats, r, g)}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    flop = 3 * 2 * d * d * n
    emit(f"    stages: {'  '.join(parts)}   (2·D²·N = {flop / 3 / 1e9:.2f} GFLOP per GEMM, three GEMMs, x3 MFMAs each)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("barlow_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"barlow_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians, fwd+bwd")
    for n, d in SHAPES:
        bench_shape(n, d, a.rounds, a.iters, emit)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
