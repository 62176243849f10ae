#!/usr/bin/env python3
"""Time of the classifier paths with --head_gemm mfma (csrc/kernels/head_gemm.hip) next to the
unchanged fma kernels and fp32 torch, in one process on one box.

  * CE head, forward + backward: B = 512, K = 2048, C in {10, 100, 1000}: mfma against fma (timed
    twice, A and B: the baseline's own spread) and against F.linear + F.cross_entropy + backward.
  * Probe / sweep training step: B = 256, K = 2048, C in {10, 100, 1000}, G in {1, 4, 8, 16}: mfma
    grouped against fma grouped (A, B) and against G back-to-back fma single steps.
  * One large-C row (C = 8192), where only mfma and torch can run.
  * Variants interleaved round by round, device events around a burst of iterations, warm-up of
    every variant first, median over the rounds. spread = max(|median A − median B|, range A, range B).
    verdict: FASTER when mfma median < min(A, B) − spread.

  python tools/head_gemm_bench.py [--out profiles/head_gemm.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

MOM, LR, WD = 0.9, 0.01, 1e-3


def timed(variants, rounds, iters, warmup=3):
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
            times[name].append(1e3 * s.elapsed_time(e) / iters)      # microseconds per call
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def cell(t):
    return f"{t[0]:9.1f} ({t[1]:7.1f}-{t[2]:7.1f})"


def spread_of(a, b):
    return max(abs(a[0] - b[0]), a[2] - a[1], b[2] - b[1])


def ce_case(m, dev, B, K, C, rounds, iters, fma_ok=True):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, K, generator=g).relu().to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    W = (torch.randn(C, K, generator=g) * 0.01).to(dev)
    b = torch.zeros(C, device=dev)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    go = torch.ones((), device=dev)

    def native(fwd, bwd):
        def run():
            lg, dz, rs, st, ls = fwd(x, W, b, y, False)
            bwd(x, dz, W, go, rs, st, ls, dW, db, True)
        return run

    Wt, bt = W.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xt = x.clone().requires_grad_(True)

    def torch_run():
        Wt.grad = bt.grad = xt.grad = None
        F.cross_entropy(F.linear(xt, Wt, bt), y).backward()

    mf = native(m.ce_head_fwd_mfma, m.ce_head_bwd_mfma)
    variants = [("mfma", mf), ("torch", torch_run)]
    if fma_ok:
        fm = native(m.ce_head_fwd, m.ce_head_bwd)
        variants = [("fmaA", fm), ("mfma", mf), ("torch", torch_run), ("fmaB", fm)]
    return timed(variants, rounds, iters)


def sweep_case(m, dev, G, B, K, C, rounds, iters, fma_ok=True):
    g = torch.Generator().manual_seed(1000 * G + C)
    x = torch.randn(B, K, generator=g).relu().to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    W0 = (torch.randn(C, K, generator=g) * 0.01).to(dev)

    def state():
        W = W0.unsqueeze(0).repeat(G, 1, 1).contiguous()
        b = torch.zeros(G, C, device=dev)
        return W, b, torch.zeros_like(W), torch.zeros_like(b)

    lrs, wds = [LR] * G, [WD] * G
    Wm, bm, uWm, ubm = state()

    def mfma():
        m.linear_ce_sweep_step_mfma(x, Wm, bm, y, uWm, ubm, lrs, MOM, wds, False, True)

    if not fma_ok:
        Wt = W0.clone().requires_grad_(True)
        bt = torch.zeros(C, device=dev, requires_grad=True)
        opt = torch.optim.SGD([Wt, bt], lr=LR, momentum=MOM, weight_decay=WD)

        def torch_run():
            for _ in range(G):
                opt.zero_grad(set_to_none=True)
                F.cross_entropy(F.linear(x, Wt, bt), y).backward()
                opt.step()

        return timed([("mfma", mfma), ("torch", torch_run)], rounds, iters)
    Wg, bg, uWg, ubg = state()
    Ws, bs, uWs, ubs = state()
    heads = [(Ws[h], bs[h], uWs[h], ubs[h]) for h in range(G)]

    def grouped():
        m.linear_ce_sweep_step(x, Wg, bg, y, uWg, ubg, lrs, MOM, wds, False, True)

    def sequential():
        for W, b, uW, ub in heads:
            m.linear_ce_step(x, W, b, y, uW, ub, LR, MOM, WD, False, True)

    r = timed([("fmaA", grouped), ("mfma", mfma), ("seq", sequential), ("fmaB", grouped)], rounds, iters)
    assert torch.isfinite(Wm).all() and torch.isfinite(Wg).all()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--heads", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--feat", type=int, default=2048)
    ap.add_argument("--large_c", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    K = a.feat
    emit(f"classifier head GEMMs: --head_gemm mfma (head_gemm.hip) against fma (linear_ce*.hip) and fp32 torch, "
         f"K = {K}, on {torch.cuda.get_device_name(0)}")
    emit(f"{a.rounds} interleaved rounds x {a.iters} calls, device events; microseconds per call: median (min-max)")
    emit("spread = the fma baseline's own: max(|median A - median B|, range A, range B); "
         "FASTER: mfma median < min(A, B) - spread")
    emit()
    emit("CE head, forward + backward, B = 512")
    emit(f"{'C':>6s} {'fma A':>28s} {'fma B':>28s} {'mfma':>28s} {'torch':>28s} {'spread':>8s} {'fma/mfma':>9s} "
         f"{'torch/mfma':>10s}  verdict")
    missed = []
    for C in a.classes:
        r = ce_case(m, dev, 512, K, C, a.rounds, a.iters)
        sp = spread_of(r["fmaA"], r["fmaB"])
        ok = r["mfma"][0] < min(r["fmaA"][0], r["fmaB"][0]) - sp
        if not ok and C == 1000:
            missed.append(f"CE head C = {C}")
        emit(f"{C:6d} {cell(r['fmaA']):>28s} {cell(r['fmaB']):>28s} {cell(r['mfma']):>28s} {cell(r['torch']):>28s} "
             f"{sp:8.1f} {r['fmaA'][0] / r['mfma'][0]:8.2f}x {r['torch'][0] / r['mfma'][0]:9.2f}x  "
             f"{'FASTER' if ok else 'not faster'}")
        flush()
    r = ce_case(m, dev, 512, K, a.large_c, a.rounds, a.iters, fma_ok=False)
    emit(f"{a.large_c:6d} {'-':>28s} {'-':>28s} {cell(r['mfma']):>28s} {cell(r['torch']):>28s} {'-':>8s} {'-':>9s} "
         f"{r['torch'][0] / r['mfma'][0]:9.2f}x  (fma cannot run)")
    emit()
    emit("probe / sweep training step, B = 256: grouped ops (fma: 2 launches, mfma: 3), G calls = G x linear_ce_step")
    emit(f"{'C':>6s} {'G':>3s} {'fma grouped A':>28s} {'fma grouped B':>28s} {'mfma grouped':>28s} {'G fma calls':>28s} "
         f"{'spread':>8s} {'fma/mfma':>9s} {'calls/mfma':>10s}  verdict")
    for C in a.classes:
        for G in a.heads:
            r = sweep_case(m, dev, G, 256, K, C, a.rounds, a.iters)
            sp = spread_of(r["fmaA"], r["fmaB"])
            ok = r["mfma"][0] < min(r["fmaA"][0], r["fmaB"][0], r["seq"][0]) - sp
            if not ok and C == 1000:
                missed.append(f"sweep C = {C} G = {G}")
            emit(f"{C:6d} {G:3d} {cell(r['fmaA']):>28s} {cell(r['fmaB']):>28s} {cell(r['mfma']):>28s} "
                 f"{cell(r['seq']):>28s} {sp:8.1f} {r['fmaA'][0] / r['mfma'][0]:8.2f}x "
                 f"{r['seq'][0] / r['mfma'][0]:9.2f}x  {'FASTER' if ok else 'not faster'}")
            flush()
    r = sweep_case(m, dev, 4, 256, K, a.large_c, a.rounds, a.iters, fma_ok=False)
    emit(f"{a.large_c:6d} {4:3d} {'-':>28s} {'-':>28s} {cell(r['mfma']):>28s} {'torch x4 ' + cell(r['torch']):>28s} "
         f"{'-':>8s} {'-':>9s} {r['torch'][0] / r['mfma'][0]:9.2f}x  (fma cannot run)")
    emit()
    emit("mfma not faster than fma by more than the spread at C = 1000: " + (", ".join(missed) if missed else "nowhere"))
    flush()


if __name__ == "__main__":
    main()
