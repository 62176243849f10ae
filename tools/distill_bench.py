#!/usr/bin/env python3
"""Cost of knowledge distillation in the supervised trainer (--distill_ckpt) -> profiles/distill.txt.

  ce     ce_head_fwd_distill[_mfma] against the soft forward op at B = 512, K = 2048,
         C = 10 / 100 / 1000.
  step   one supervised ResNet-50 CIFAR step (256 images, bf16, eager): flags off, flags off
         again (the baseline's own spread), a ResNet-50 teacher, and — with --parent TREE, a built
         checkout of the parent commit — flags off on that tree. Every measurement of this part is
         a fresh child process (its own engine), the variants interleaved round by round. The
         teacher step stands next to the FoldedEncoder forward of the same batch alone.

Interleaved rounds, device events around a burst of iterations, median and range over the rounds;
a row slower than its baseline beyond the baseline's own spread is printed in bold (**...**).

  python tools/distill_bench.py [--parts ce step] [--parent TREE] [--out profiles/distill.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


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


def bench_ce(a, out):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    dev = torch.device("cuda:0")
    B, K = 512, 2048
    out(f"forward op, B = {B}, K = {K}, temp 2, alpha 0.5; microseconds (median, min-max); x = against the soft op")
    for C in (10, 100, 1000):
        torch.manual_seed(C)
        x = torch.randn(B, K, device=dev).relu()
        W = torch.randn(C, K, device=dev) / K ** 0.5
        b = torch.zeros(C, device=dev)
        y = torch.randint(0, C, (B,), device=dev)
        y2 = y.roll(1)
        v = 3 * torch.randn(B, C, device=dev)
        for tag, soft, distill in (("fma", m.ce_head_fwd_soft, m.ce_head_fwd_distill),
                                   ("mfma", m.ce_head_fwd_soft_mfma, m.ce_head_fwd_distill_mfma)):
            r = timed([("soft", lambda: soft(x, W, b, y, y2, 0.3, 0.1, True)),
                       ("soft again", lambda: soft(x, W, b, y, y2, 0.3, 0.1, True)),
                       ("distill", lambda: distill(x, W, b, y, y2, 0.3, 0.1, v, 2.0, 0.5, True)),
                       ("distill alpha 1", lambda: distill(x, W, b, y, y2, 1.0, 0.0, v, 2.0, 1.0, True))],
                      a.rounds, a.iters)
            spread = abs(r["soft again"][0] - r["soft"][0])
            for n in ("soft", "soft again", "distill", "distill alpha 1"):
                out("  " + row(f"C = {C:4d} {tag:4s} {n}", r[n], r["soft"][0] if n != "soft" else None, spread))


STEP_CHILD = r"""
import sys, tempfile, torch
from simclr_pytorch_distributed_amd.config import parse_ce
from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
iters, extra = int(sys.argv[1]), sys.argv[2:]
dev = torch.device("cuda:0")
eng = SupervisedEngine(parse_ce(["--model", "resnet50", "--backend", "native", "--synthetic", "--synthetic_size", "1024",
                                 "--batch_size", "256", "--work_dir", tempfile.mkdtemp(prefix="distill_step_"), *extra]),
                       device=dev)
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
if getattr(eng, "teacher", None) is not None:
    x = eng.make_views(idx, 1, 0)
    for _ in range(5):
        eng._teacher_encode(x)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        eng._teacher_encode(x)
    e.record()
    torch.cuda.synchronize()
    print("ENC_MS", s.elapsed_time(e) / iters)
"""


def write_teacher(path):
    """A ResNet-50 checkpoint of the supervised trainer's layout with fresh weights: the cost of the
    teacher does not depend on what it has learned."""
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    torch.manual_seed(0)
    torch.save({"opt": {}, "model": ckpt_mod.model_state_with_prefix(SupCEResNet("resnet50", 10)), "optimizer": {},
                "epoch": 1}, path)


def bench_step(a, out):
    ck = os.path.join(tempfile.mkdtemp(prefix="distill_bench_"), "teacher.pth")
    write_teacher(ck)
    on = ["--distill_ckpt", ck, "--distill_temp", "2", "--distill_alpha", "0.5"]
    variants = [("flags off", ROOT, []), ("flags off again", ROOT, []), ("resnet50 teacher", ROOT, on)]
    if a.parent:
        variants.insert(1, ("parent commit, flags off", os.path.abspath(a.parent), []))
    times = {n: [] for n, _, _ in variants}
    enc = []
    for _ in range(a.step_rounds):
        for name, tree, extra in variants:
            env = dict(os.environ, PYTHONPATH=tree, SDX_AUTOBUILD="0")
            r = subprocess.run([sys.executable, "-c", STEP_CHILD, str(a.step_iters), *extra], env=env, cwd=tree,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: child failed\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
            times[name].append(float(r.stdout.split("STEP_MS")[1].split()[0]))
            print(f"  [{name}] {times[name][-1]:.3f} ms", file=sys.stderr, flush=True)
            if "ENC_MS" in r.stdout:
                enc.append(float(r.stdout.split("ENC_MS")[1].split()[0]))
    r = {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}
    spread = abs(r["flags off again"][0] - r["flags off"][0])
    out(f"one supervised step, resnet50 CIFAR stem, 256 images, bf16, eager; {a.step_rounds} interleaved rounds of fresh "
        f"processes x {a.step_iters} steps; milliseconds (median, min-max); teacher = {' '.join(on[2:])}")
    base = r["parent commit, flags off"][0] if a.parent else r["flags off"][0]
    for name, _, _ in variants:
        first = name == ("parent commit, flags off" if a.parent else "flags off")
        out("  " + row(name, r[name], None if first else base, spread, unit=1.0))
    out(f"  the baseline's own spread (flags off against flags off again): {spread:.3f} ms")
    e = (statistics.median(enc), min(enc), max(enc))
    out("  " + row("FoldedEncoder forward alone, same batch", e, None, unit=1.0))
    out(f"  teacher step - flags off: {r['resnet50 teacher'][0] - r['flags off'][0]:.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", dest="what", nargs="+", default=["ce", "step"], choices=["ce", "step"])
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (step part)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--step_iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"tools/distill_bench.py {' '.join(a.what)}; {a.rounds} interleaved rounds x {a.iters} iterations; "
        f"{torch.cuda.get_device_name(0)}")
    for what in a.what:
        out("")
        {"ce": bench_ce, "step": bench_step}[what](a, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
