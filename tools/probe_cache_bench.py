#!/usr/bin/env python3
"""Time of the linear probe with --cache_features, in one process on one box.

  (a) Per classifier step, B = 256, K = 2048, C in {10, 100, 1000}, fma and mfma, on a 50 000-row
      bank and a fresh random index batch per call. G = 1: the single-head ops the default probe
      runs (linear_ce_step[_mfma][_rows]); G = 8: the sweep ops. The row-indexed op (rows) against
      torch.index_select of features and labels followed by the plain op (gatherA / gatherB: the
      baseline timed twice, its own spread). Variants interleaved round by round, device events
      around a burst of calls, warm-up of every variant first, median over the rounds.
      spread = max(|median A − median B|, range A, range B); verdict FASTER / SLOWER when the rows
      median lies outside min / max(A, B) by more than the spread, else same.
  (b) Per epoch, ResNet-50 on synthetic CIFAR-sized data (50 000 / 10 000, batch 256): wall time of
      train_epoch + validate for --cache_features off, val and all (host clock around a device
      synchronise), epochs interleaved over the three engines, and the one-off extraction time.

  python tools/probe_cache_bench.py [--out profiles/probe_cache.txt] [--skip_epoch]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.head_gemm_bench import cell, spread_of, timed

MOM, LR, WD = 0.9, 0.01, 1e-3
N_BANK, B, K = 50000, 256, 2048


def step_case(m, dev, gemm, G, C, rounds, iters):
    g = torch.Generator().manual_seed(100 * G + C)
    bank = torch.randn(N_BANK, K, generator=g).relu().to(dev)
    labels = torch.randint(0, C, (N_BANK,), generator=g).to(dev)
    # a ring of index batches, so that consecutive calls read different bank rows
    ring = [torch.randint(0, N_BANK, (B,), generator=g).to(dev) for _ in range(64)]
    # G = 1: the single-head ops (NativeLinearCE); G > 1: the sweep ops (NativeLinearSweep)
    name = ("linear_ce_step" if G == 1 else "linear_ce_sweep_step") + ("_mfma" if gemm == "mfma" else "")
    plain, rows_op = getattr(m, name), getattr(m, name + "_rows")
    lrs, wds = (LR, WD) if G == 1 else ([LR] * G, [WD] * G)
    lead = () if G == 1 else (G,)

    def state():
        W = (torch.randn(*lead, C, K, generator=g) * 0.01).to(dev)
        b = torch.zeros(*lead, C, device=dev)
        return W, b, torch.zeros_like(W), torch.zeros_like(b)

    sr, sg = state(), state()
    pos = [0, 0]

    def rows():
        r = ring[pos[0] % 64]
        pos[0] += 1
        rows_op(bank, sr[0], sr[1], labels, r, sr[2], sr[3], lrs, MOM, wds, False, True)

    def gather():
        r = ring[pos[1] % 64]
        pos[1] += 1
        plain(torch.index_select(bank, 0, r), sg[0], sg[1], torch.index_select(labels, 0, r), sg[2], sg[3], lrs, MOM,
              wds, False, True)

    return timed([("gatherA", gather), ("rows", rows), ("gatherB", gather)], rounds, iters)


def epoch_case(dev, epochs, lines):
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    import tempfile
    engines = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("off", "val", "all"):
            argv = ["--model", "resnet50", "--backend", "native", "--synthetic", "--synthetic_size", "50000",
                    "--batch_size", "256", "--val_batch_size", "256", "--epochs", str(epochs), "--print_freq", "1000",
                    "--learning_rate", "1", "--work_dir", os.path.join(tmp, mode), "--cache_features", mode]
            engines[mode] = LinearEngine(parse_linear(argv, make_dirs=True), device=dev)
        extract = {}
        for mode, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.prepare_cache()
            torch.cuda.synchronize()
            extract[mode] = time.perf_counter() - t0
        times = {mode: [] for mode in engines}
        for epoch in range(1, epochs + 1):
            for mode, e in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.train_epoch(epoch)
                e.validate()
                torch.cuda.synchronize()
                times[mode].append(time.perf_counter() - t0)
    lines.append(f"(b) epoch = train_epoch + validate, ResNet-50, synthetic 50000 / {len(engines['off'].val)}, batch 256, "
                 f"{epochs} epochs interleaved, the first dropped as warm-up; seconds")
    lines.append(f"{'mode':>5} {'median':>8} {'min':>8} {'max':>8} {'extraction (once)':>18}")
    for mode, t in times.items():
        t = t[1:]
        lines.append(f"{mode:>5} {statistics.median(t):8.3f} {min(t):8.3f} {max(t):8.3f} {extract[mode]:18.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--skip_epoch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_cache_bench measures on the GPU: none found")
    from simclr_pytorch_distributed_amd.ops import _ext
    m, dev = _ext.require(), torch.device("cuda:0")
    lines = [f"probe_cache_bench: {torch.cuda.get_device_name(0)}, rounds {a.rounds} x {a.iters} calls",
             f"(a) training step on a {N_BANK}-row bank, B = {B}, K = {K} (G = 1: linear_ce_step[_mfma], G = 8: "
             f"linear_ce_sweep_step[_mfma]); microseconds per step, median (min-max)",
             f"{'gemm':>5} {'G':>3} {'C':>5} {'gatherA':>28} {'rows':>28} {'gatherB':>28} {'spread':>8}  verdict"]
    for gemm in ("fma", "mfma"):
        for G in (1, 8):
            for C in (10, 100, 1000):
                t = step_case(m, dev, gemm, G, C, a.rounds, a.iters)
                sp = spread_of(t["gatherA"], t["gatherB"])
                lo, hi = min(t["gatherA"][0], t["gatherB"][0]), max(t["gatherA"][0], t["gatherB"][0])
                verdict = "FASTER" if t["rows"][0] < lo - sp else ("SLOWER" if t["rows"][0] > hi + sp else "same")
                lines.append(f"{gemm:>5} {G:3d} {C:5d} {cell(t['gatherA'])} {cell(t['rows'])} {cell(t['gatherB'])} "
                             f"{sp:8.1f}  {verdict}")
                print(lines[-1], flush=True)
    if not a.skip_epoch:
        epoch_case(dev, a.epochs, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
