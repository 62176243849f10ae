#!/usr/bin/env python3
"""Time of one linear-probe SWEEP training step (G classifiers on one feature batch, op
linear_ce_sweep_step: two launches) next to the same work as G back-to-back linear_ce_step calls
(2·G launches) on the same tensors, and of the frozen encoder's forward for scale.

  * B = 256 rows of K = 2048 features, C in {10, 100, 1000}, G in {1, 4, 8, 16}, fp32.
  * Three variants interleaved in one process: the G calls, the grouped step, the G calls again.
    The two runs of the G calls are the baseline's own run-to-run spread: the larger of the
    distance of their medians and of either run's min-max range.
  * Device events around a burst of iterations, warm-up of every variant first, median over rounds.
  * The FoldedEncoder ResNet-50 forward of 256 CIFAR-sized images (bf16) is timed the same way.

  python tools/probe_sweep_bench.py [--out profiles/probe_sweep.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MOM, LR, WD = 0.9, 0.01, 1e-3


def timed(variants, rounds, iters, warmup=5):
    for _, fn in variants:
        for _ in range(warmup):
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
            times[name].append(1e3 * s.elapsed_time(e) / iters)      # microseconds per step
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def sweep_case(m, dev, G, B, K, C, rounds, iters):
    g = torch.Generator().manual_seed(1000 * G + C)
    x = torch.randn(B, K, generator=g).relu().to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    W0 = (torch.randn(C, K, generator=g) * 0.01).to(dev)

    def state():
        W = W0.unsqueeze(0).repeat(G, 1, 1).contiguous()
        b = torch.zeros(G, C, device=dev)
        return W, b, torch.zeros_like(W), torch.zeros_like(b)

    Ws, bs, uWs, ubs = state()           # the G calls work on the heads of one stacked tensor
    Wg, bg, uWg, ubg = state()
    heads = [(Ws[h], bs[h], uWs[h], ubs[h]) for h in range(G)]
    lrs, wds = [LR] * G, [WD] * G

    def sequential():
        for W, b, uW, ub in heads:
            m.linear_ce_step(x, W, b, y, uW, ub, LR, MOM, WD, False, True)

    def grouped():
        m.linear_ce_sweep_step(x, Wg, bg, y, uWg, ubg, lrs, MOM, wds, False, True)

    sequential()
    grouped()
    torch.cuda.synchronize()
    assert torch.equal(Ws, Wg) and torch.equal(uWs, uWg), "the grouped step and the G calls disagree"
    r = timed([("seq", sequential), ("grouped", grouped), ("seq2", sequential)], rounds, iters)
    assert torch.isfinite(Ws).all() and torch.isfinite(Wg).all()
    return r


def encoder_case(dev, images, rounds, iters):
    from simclr_pytorch_distributed_amd.models.executor import to_nhwc_input
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.ops.linear_probe import FoldedEncoder
    torch.manual_seed(0)
    model = SupConResNet("resnet50").to(dev).to(memory_format=torch.channels_last).eval()
    enc = FoldedEncoder(model.encoder)
    x = to_nhwc_input(torch.randn(images, 3, 32, 32, device=dev))
    return timed([("encoder", lambda: enc(x))], rounds, iters)["encoder"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--feat", type=int, default=2048)
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    B, K = a.batch, a.feat
    emit(f"linear-probe sweep: one training step of G classifiers, fp32, B = {B}, K = {K}, on "
         f"{torch.cuda.get_device_name(0)}")
    emit(f"grouped = linear_ce_sweep_step (2 launches); G calls = G x linear_ce_step (2·G launches) on the same "
         f"tensors, timed twice (A, B)")
    emit(f"{a.rounds} interleaved rounds x {a.iters} steps, device events; microseconds per step: median (min-max)")
    emit(f"spread = baseline's own: max(|median A - median B|, range A, range B); "
         f"verdict: grouped median against the slower-or-equal rule grouped <= min(A, B) + spread")
    emit(f"{'C':>5s} {'G':>3s} {'G calls A':>24s} {'G calls B':>24s} {'grouped':>24s} {'spread':>8s} "
         f"{'A / grouped':>12s}  verdict")
    slower = []
    for C in a.classes:
        for G in a.heads:
            r = sweep_case(m, dev, G, B, K, C, a.rounds, a.iters)
            s1, s2, gr = r["seq"], r["seq2"], r["grouped"]
            spread = max(abs(s1[0] - s2[0]), s1[2] - s1[1], s2[2] - s2[1])
            ok = gr[0] <= min(s1[0], s2[0]) + spread
            if not ok:
                slower.append((C, G))

            def cell(t):
                return f"{t[0]:9.1f} ({t[1]:6.1f}-{t[2]:6.1f})"

            emit(f"{C:5d} {G:3d} {cell(s1):>24s} {cell(s2):>24s} {cell(gr):>24s} {spread:8.1f} "
                 f"{s1[0] / gr[0]:11.2f}x  {'not slower' if ok else 'SLOWER'}")
    enc = encoder_case(dev, B, a.rounds, max(5, a.iters // 5))
    emit()
    emit(f"FoldedEncoder ResNet-50 (CIFAR stem, bf16) forward of {B} 32x32 images: "
         f"{enc[0] / 1e3:.3f} ms ({enc[1] / 1e3:.3f}-{enc[2] / 1e3:.3f})")
    emit("grouped step slower than the G calls by more than the spread at (C, G): "
         + (", ".join(f"({c}, {g})" for c, g in slower) if slower else "nowhere"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
