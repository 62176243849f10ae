#!/usr/bin/env python3
"""Time of the augmentation launch alone, with and without the Gaussian-blur stage.

Shape of bench.py --config supcon224 (config 5): 512 images x 2 views at 224x224 from a
native-resolution ragged store. Variants: blur_p 0 (the plain kernel), 0.5 and 1 with the
automatic rows per barrier round, and blur_p 1 at explicit rows per round. The variants are
timed in interleaved rounds in one process (device events around a burst of launches, median
and range over the rounds), so drift of the box hits all of them alike.

  python tools/aug_blur_bench.py [--batch 512] [--size 224] [--rounds 9] [--iters 40]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simclr_pytorch_distributed_amd.data.augment import AugConfig, blur_plan, gpu_augment

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def ragged_store(n, side, seed, dev):
    """n random images of about side x 1.25 side (ImageFolder-like native resolutions)."""
    r = np.random.default_rng(seed)
    shapes = [(int(side * r.uniform(1.0, 1.3)), int(side * r.uniform(1.0, 1.5))) for _ in range(n)]
    sizes = [h * w * 3 for h, w in shapes]
    data = torch.from_numpy(r.integers(0, 256, sum(sizes), dtype=np.uint8))
    offs = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64)
    return data.to(dev), offs.to(dev), torch.tensor(shapes, dtype=torch.int32).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 2, 4, 8])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    data, offs, hw = ragged_store(a.images, int(a.size * 256 / 224), 0, dev)
    idx = torch.from_numpy(np.random.default_rng(1).permutation(a.images)[:a.batch]).to(dev)

    variants = [("blur_p=0 (aug_kernel)", AugConfig.simclr(a.size, MEAN, STD), 0)]
    for p in (0.5, 1.0):
        variants.append((f"blur_p={p} rows=auto", AugConfig.simclr(a.size, MEAN, STD, blur_p=p), 0))
    for rows in a.rows:
        cfg = AugConfig.simclr(a.size, MEAN, STD, blur_p=1.0)
        if blur_plan(a.size, cfg.blur_k, rows) is not None:
            variants.append((f"blur_p=1.0 rows={rows}", cfg, rows))
    plan = blur_plan(a.size)
    print(f"shape: {a.batch} images x 2 views, S={a.size}, k={plan['k']}; automatic plan: rows={plan['rows']} "
          f"strips={plan['n_strips']} LDS={plan['lds_bytes']} B; {a.rounds} interleaved rounds x {a.iters} launches",
          flush=True)

    def launch(cfg, rows, seed):
        return gpu_augment(data, idx, cfg, seed, offs=offs, hw=hw, _blur_rows=rows)

    for _, cfg, rows in variants:          # warm up every variant
        for s in range(2):
            launch(cfg, rows, s)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for rnd in range(a.rounds):
        for name, cfg, rows in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for it in range(a.iters):
                launch(cfg, rows, 1000 * rnd + it)     # the same seeds for every variant
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.iters)
    base = statistics.median(times[variants[0][0]])
    print(f"{'variant':26s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'added ms':>9s}")
    for name, _, _ in variants:
        t = times[name]
        med = statistics.median(t)
        print(f"{name:26s} {med:10.3f} {min(t):8.3f} {max(t):8.3f} {med - base:9.3f}", flush=True)


if __name__ == "__main__":
    main()
