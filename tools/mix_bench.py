#!/usr/bin/env python3
"""Cost of Mixup / CutMix / label smoothing in the supervised trainer -> profiles/mix.txt.

  mix    the mix_views launch alone (mixup, cutmix) at 256 x 32² and 512 x 224², next to the
         augmentation launch that produces the batch at the same shape.
  ce     ce_head_fwd_soft[_mfma] against the plain forward op at B = 512, K = 2048,
         C = 10 / 100 / 1000.
  step   one supervised ResNet-50 CIFAR step (256 images, bf16, eager): flags off, flags off
         again (the baseline's own spread), flags on, and — with --parent TREE, a built checkout of
         the parent commit — flags off on that tree. Every measurement of this part is a fresh
         child process (its own engine), the variants interleaved round by round.

Interleaved rounds, device events around a burst of iterations, median and range over the rounds;
a row slower than its baseline beyond the baseline's own spread is printed in bold (**...**).

  python tools/mix_bench.py [--parts mix ce step] [--parent TREE] [--out profiles/mix.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

FLAGS_ON = ["--mixup", "0.8", "--cutmix", "1.0", "--label_smoothing", "0.1"]


def timed(variants, rounds, iters):
    for _, fn in variants:
        for _ in range(3):
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
            times[name].append(s.elapsed_time(e) / iters)
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def row(name, m, base=None, spread=0.0, unit=1e3):
    txt = f"{name:44s} {unit * m[0]:10.2f} ({unit * m[1]:.2f}-{unit * m[2]:.2f})"
    if base is not None:
        txt += f"  {m[0] / base:6.3f}x"
        if m[0] > base + spread:
            txt = f"**{txt}**"
    return txt


def bench_mix(a, out):
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, gpu_augment, mix_views
    dev = torch.device("cuda:0")
    out("mix_views alone next to the augmentation launch; microseconds (median, min-max); x = against the augmentation")
    for B, S in ((256, 32), (512, 224)):
        data = torch.randint(0, 256, (max(B, 1024), S, S, 3), dtype=torch.uint8, device=dev)
        idx = torch.arange(B, device=dev)
        cfg = AugConfig.linear_train(S, (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))
        x = gpu_augment(data, idx, cfg, 1)
        q = S // 4
        r = timed([("aug", lambda: gpu_augment(data, idx, cfg, 1)), ("aug again", lambda: gpu_augment(data, idx, cfg, 1)),
                   ("mixup", lambda: mix_views(x, "mixup", 0.3)),
                   ("cutmix", lambda: mix_views(x, "cutmix", 0.75, q, 3 * q, q, 3 * q))], a.rounds, a.iters)
        spread = abs(r["aug again"][0] - r["aug"][0])
        out(f"  {B} x {S}x{S} ({B * S * S * 16 / 2 ** 20:.0f} MiB)")
        for n in ("aug", "aug again", "mixup", "cutmix"):
            out("  " + row(f"{n}", r[n], r["aug"][0] if n != "aug" else None, spread))


def bench_ce(a, out):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    dev = torch.device("cuda:0")
    B, K = 512, 2048
    out(f"forward op, B = {B}, K = {K}; microseconds (median, min-max); x = against the plain op")
    for C in (10, 100, 1000):
        torch.manual_seed(C)
        x = torch.randn(B, K, device=dev).relu()
        W = torch.randn(C, K, device=dev) / K ** 0.5
        b = torch.zeros(C, device=dev)
        y = torch.randint(0, C, (B,), device=dev)
        y2 = y.roll(1)
        for tag, plain, soft in (("fma", m.ce_head_fwd, m.ce_head_fwd_soft),
                                 ("mfma", m.ce_head_fwd_mfma, m.ce_head_fwd_soft_mfma)):
            r = timed([("plain", lambda: plain(x, W, b, y, True)), ("plain again", lambda: plain(x, W, b, y, True)),
                       ("soft", lambda: soft(x, W, b, y, y2, 0.3, 0.1, True))], a.rounds, a.iters)
            spread = abs(r["plain again"][0] - r["plain"][0])
            for n in ("plain", "plain again", "soft"):
                out("  " + row(f"C = {C:4d} {tag:4s} {n}", r[n], r["plain"][0] if n != "plain" else None, spread))


STEP_CHILD = r"""
import sys, tempfile, torch
from simclr_pytorch_distributed_amd.config import parse_ce
from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
iters, extra = int(sys.argv[1]), sys.argv[2:]
dev = torch.device("cuda:0")
eng = SupervisedEngine(parse_ce(["--model", "resnet50", "--backend", "native", "--synthetic", "--synthetic_size", "1024",
                                 "--batch_size", "256", "--work_dir", tempfile.mkdtemp(prefix="mix_step_"), *extra]), device=dev)
eng.model.train()
idx = torch.arange(256, device=dev)
labels = eng.train.labels[idx]
for it in range(5):
    eng.train_step(idx, labels, 1, it, 100)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for it in range(iters):
    eng.train_step(idx, labels, 1, 5 + it, 100)
e.record()
torch.cuda.synchronize()
print("STEP_MS", s.elapsed_time(e) / iters)
"""


def bench_step(a, out):
    variants = [("flags off", ROOT, []), ("flags off again", ROOT, []), ("flags on", ROOT, FLAGS_ON)]
    if a.parent:
        variants.insert(1, ("parent commit, flags off", os.path.abspath(a.parent), []))
    times = {n: [] for n, _, _ in variants}
    for _ in range(a.step_rounds):
        for name, tree, extra in variants:
            env = dict(os.environ, PYTHONPATH=tree, SDX_AUTOBUILD="0")
            r = subprocess.run([sys.executable, "-c", STEP_CHILD, str(a.step_iters), *extra], env=env, cwd=tree,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: child failed\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
            times[name].append(float(r.stdout.split("STEP_MS")[1].split()[0]))
    r = {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}
    spread = abs(r["flags off again"][0] - r["flags off"][0])
    out(f"one supervised step, resnet50 CIFAR stem, 256 images, bf16, eager; {a.step_rounds} interleaved rounds of fresh "
        f"processes x {a.step_iters} steps; milliseconds (median, min-max); flags on = {' '.join(FLAGS_ON)}")
    base = r["parent commit, flags off"][0] if a.parent else r["flags off"][0]
    for name, _, _ in variants:
        first = name == ("parent commit, flags off" if a.parent else "flags off")
        out("  " + row(name, r[name], None if first else base, spread, unit=1.0))
    out(f"  the baseline's own spread (flags off against flags off again): {spread:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", dest="what", nargs="+", default=["mix", "ce", "step"], choices=["mix", "ce", "step"])
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (step part)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--step_iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"tools/mix_bench.py {' '.join(a.what)}; {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"{torch.cuda.get_device_name(0)}")
    for what in a.what:
        out("")
        {"mix": bench_mix, "ce": bench_ce, "step": bench_step}[what](a, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
