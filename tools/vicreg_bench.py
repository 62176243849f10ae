#!/usr/bin/env python3
"""VICReg loss: the native kernels (csrc/kernels/vicreg.hip) against the fp32 torch twin
(losses/vicreg.py vicreg_reference), and vic_cov against the general product it replaces, on the
same GPU.

Every (N, D) is warmed up, then timed in interleaved rounds baseline, native, baseline: the two
baseline series give the baseline's own spread. A round is ``--iters`` calls between two device
events; medians over ``--rounds``.

* forward + backward, native against the twin;
* ``vic_cov`` (both views, T(T + 1)/2 tiles each) against two calls of ``barlow_xcorr(z_v, z_v, …)``
  (T² tiles each, both operands standardised): the tile count predicts (T + 1)/(2T) of that time;
* the stage ops singly (device events around one op: launch gaps included).

``--stage_check`` prints the worst error / bound of the GEMM stages against fp64 at the test shapes
(the bounds of tests/test_gpu_vicreg.py). Needs a GPU; there is no CPU fall-back.

    python tools/vicreg_bench.py [--rounds 7] [--iters 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from loss_bench_common import interleaved, med, timed  # noqa: E402
from simclr_pytorch_distributed_amd.losses.vicreg import vicreg_reference  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext, vicreg  # noqa: E402

SHAPES = [(n, d) for n in (256, 1024) for d in (128, 2048, 8192)]
W, EPS = (25.0, 25.0, 1.0), 1e-4


def fwd_bwd(loss_fn, z1, z2):
    def run():
        z1.grad = z2.grad = None
        loss_fn(z1, z2, *W, EPS).backward()
    return run


def bench_shape(n, d, rounds, iters, emit):
    m = _ext.require()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n + d)
    z1 = torch.randn(n, d, device=dev, generator=gen).requires_grad_(True)
    z2 = (0.5 * z1.detach() + torch.randn(n, d, device=dev, generator=gen)).requires_grad_(True)
    twin, native = fwd_bwd(vicreg_reference, z1, z2), fwd_bwd(vicreg.vicreg_loss, z1, z2)
    # same inputs, same result (fp32 twin: tolerance of its own GEMMs)
    twin()
    gt = z1.grad.clone()
    native()
    rel = ((z1.grad - gt).abs().max() / gt.abs().max()).item()
    a, b, nat, lo, hi = interleaved(twin, native, rounds, iters)
    slower = nat > min(a, b)
    emit(f"N={n:5d} D={d:5d}  twin {a:8.3f} / {b:8.3f} ms (two series)  native {nat:8.3f} ms [{lo:.3f} .. {hi:.3f}]  "
         f"twin/native {0.5 * (a + b) / nat:5.2f}x{'  NATIVE SLOWER' if slower else ''}  grad diff/max {rel:.2e}")
    # vic_cov against the general product
    a1, a2 = z1.detach(), z2.detach()
    sums, mu = m.vicreg_colstats(a1, a2)
    stats = m.barlow_colstats(a1, a2, 1e-5)[1]
    s11 = torch.cat([stats[0], stats[0]]).reshape(2, 2, d).contiguous()
    s22 = torch.cat([stats[1], stats[1]]).reshape(2, 2, d).contiguous()

    def general():
        m.barlow_xcorr(a1, a1, s11)
        m.barlow_xcorr(a2, a2, s22)

    ga, gb, cv, lo, hi = interleaved(general, lambda: m.vicreg_cov(a1, a2, mu), rounds, iters)
    T = -(-d // 128)
    pred, meas, spread = (T + 1) / (2 * T), cv / (0.5 * (ga + gb)), abs(ga - gb) / (0.5 * (ga + gb))
    emit(f"    vic_cov {cv * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  2 x bt_xcorr {ga * 1e3:8.1f} / {gb * 1e3:8.1f} us"
         f"  ratio {meas:.3f} (tile count predicts {pred:.3f}; baseline spread {spread:.3f})"
         f"{'  ABOVE PREDICTION' if meas > pred + spread else ''}")
    # stages, one op each
    C = m.vicreg_cov(a1, a2, mu)
    C0 = C.clone()
    _, _, G, coef = m.vicreg_loss_grad(C0.clone(), sums, *W, EPS, n)
    g = torch.ones(1, device=dev)
    stages = {"vic_colstats": lambda: m.vicreg_colstats(a1, a2),
              "vic_cov": lambda: m.vicreg_cov(a1, a2, mu),
              "copy of C": lambda: C.copy_(C0),     # the in-place stage needs a fresh C per call:
              "copy + vic_loss_grad + finish": lambda: m.vicreg_loss_grad(C.copy_(C0), sums, *W, EPS, n),   # subtract the copy
              "vic_bwd": lambda: m.vicreg_bwd(a1, a2, G, mu, coef, g, W[0])}
    parts = []
    for name, fn in stages.items():
        fn()
        parts.append(f"{name} {med([timed(fn, iters) for _ in range(rounds)]) * 1e3:.1f} us")
    emit(f"    stages: {'  '.join(parts)}   (2·D²·N = {2 * d * d * n / 1e9:.2f} GFLOP per full GEMM, x3 MFMAs each)")


def stage_check(emit):
    """Worst error / bound of the two GEMM stages against fp64 of their own inputs."""
    m = _ext.require()
    dev = torch.device("cuda:0")
    u, eps_p = 2.0 ** -24, 2.0 ** -16
    for n, d in ((8, 64), (40, 192), (264, 320), (64, 2048)):
        gen = torch.Generator().manual_seed(31 * n + d)
        scale = 10.0 ** (2 * torch.rand(d, generator=gen, dtype=torch.float64) - 1)
        z1 = (torch.randn(n, d, generator=gen, dtype=torch.float64) * scale + scale * 3).float()
        z2 = (0.5 * z1.double() + torch.randn(n, d, generator=gen, dtype=torch.float64) * scale).float()
        a1, a2 = z1.to(dev), z2.to(dev)
        sums, mu = m.vicreg_colstats(a1, a2)
        C = m.vicreg_cov(a1, a2, mu)
        C0 = C.cpu().double()
        _, _, G, coef = m.vicreg_loss_grad(C, sums, *W, EPS, n)
        dz = m.vicreg_bwd(a1, a2, G, mu, coef, torch.ones(1, device=dev), 0.0)
        mu64, G64, coef64 = mu.cpu().double(), G.cpu().double(), coef.cpu().double()
        rc = rb = 0.0
        for v, z in enumerate((z1.double(), z2.double())):
            x = z - mu64[v]
            bound = (eps_p + n * u + 4 * u) * (x.abs().t() @ x.abs() / (n - 1))
            rc = max(rc, ((C0[v] - x.t() @ x / (n - 1)).abs() / (bound + 1e-300)).max().item())
            a, b = x @ G64[v], coef64[v] * x
            bound = (eps_p + d * u + 2 * u) * (x.abs() @ G64[v].abs()) + 6 * u * (a.abs() + b.abs())
            rb = max(rb, ((dz[v].cpu().double() - (a - b)).abs() / (bound + 1e-300)).max().item())
        emit(f"stage check N={n:4d} D={d:5d}: C error/bound {rc:.3f}  dz error/bound {rb:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stage_check", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vicreg_bench needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"vicreg_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x iters {a.iters}, medians")
    for n, d in SHAPES:
        bench_shape(n, d, a.rounds, a.iters, emit)
    if a.stage_check:
        stage_check(emit)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
