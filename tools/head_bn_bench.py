#!/usr/bin/env python3
"""One hidden layer of the BatchNorm projector head (Linear -> BatchNorm1d -> ReLU, training mode):
the fused column-strip kernels of csrc/kernels/head_bn.hip against

* composed: the same layer from the project's existing ops: the 1x1 forward GEMM with the
  BN-statistics epilogue, the statistics reduction, finalize + the apply kernel (ops/conv.py,
  ops/bn.py), forward only;
* torch:    autocast-bf16 ``Linear + BatchNorm1d + ReLU``, forward only.

Every shape is warmed up, then timed in interleaved rounds baseline, fused, baseline: the two
baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``. The backward kernel (hbn_bwd: BN + ReLU backward with dγ, dβ) is
timed alone; both baselines run that stage inside larger backward chains. Needs a GPU.

    python tools/head_bn_bench.py [--rounds 7] [--iters 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext  # noqa: E402
from simclr_pytorch_distributed_amd.ops.bn import bn_act  # noqa: E402

SHAPES = [(512, 2048, 2048), (512, 2048, 8192), (512, 8192, 8192), (128, 2048, 2048), (2048, 2048, 2048)]


def bench_shape(n, k, h, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + k + h)
    x = torch.randn(n, k, device=dev, generator=gen).bfloat16()
    lin = torch.nn.Linear(k, h, bias=False).to(dev)
    bn1, bn2 = torch.nn.BatchNorm1d(h).to(dev), torch.nn.BatchNorm2d(h).to(dev)
    w = lin.weight.detach().bfloat16().contiguous()
    g, b = bn1.weight.detach(), bn1.bias.detach()
    rm, rv = torch.zeros(h, device=dev), torch.ones(h, device=dev)
    x4, w4 = x.view(n, 1, 1, k), w.view(h, 1, 1, k)
    xf = x.float()

    def fused():
        return m.head_bn_layer_fwd(x, w, g, b, rm, rv, 0.1, 1e-5)

    def composed():
        y, slab = m.conv_fwd(x4, w4, 1, 0, True, -1)
        return bn_act(y, m.bn_stats_reduce(slab), bn2, True, True, None)

    def torch_fwd():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return torch.relu(bn1(lin(xf)))

    with torch.no_grad():
        a, yb, mu, rstd = fused()
        ta, tb, fu, lo, hi = interleaved(torch_fwd, fused, rounds, iters)
        if h <= 4096:     # the BN kernels of the composed chain stop at 4096 channels
            diff = (a.float() - composed().view(n, h).float()).abs().max().item()
            ca, cb, fu, lo, hi = interleaved(composed, fused, rounds, iters)
        da = torch.randn(n, h, device=dev, generator=gen).bfloat16()
        sg, sb = torch.zeros(h, device=dev), torch.zeros(h, device=dev)
        bwd = med([timed(lambda: m.head_bn_layer_bwd(da, yb, mu, rstd, g, b, sg, sb), iters) for _ in range(rounds)])
    comp = "composed        - (H > 4096)"
    if h <= 4096:
        comp = (f"composed {ca * 1e3:8.1f} / {cb * 1e3:8.1f} us ({0.5 * (ca + cb) / fu:5.2f}x"
                f"{', FUSED SLOWER' if fu > max(ca, cb) else ''}; max |a - composed| {diff:.3g})")
    emit(f"N={n:5d} K={k:5d} H={h:5d}  fused fwd {fu * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {comp}  "
         f"torch {ta * 1e3:8.1f} / {tb * 1e3:8.1f} us{'  FUSED SLOWER THAN TORCH' if fu > max(ta, tb) else ''}  "
         f"hbn_bwd {bwd * 1e3:7.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_bn_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"head_bn_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians")
    for n, k, h in SHAPES:
        bench_shape(n, k, h, a.rounds, a.iters, emit)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
