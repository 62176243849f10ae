#!/usr/bin/env python3
"""Time of the evaluation transform (Resize + CenterCrop + normalize) next to the encoder it feeds.

Workload: a batch of images from a ragged store with sides drawn like ImageNet's (shorter side
333-500 px before the native store's cap of 2.58 x size, aspect up to 3:2), -> (256, 224). Three
things are timed in interleaved rounds in one process (device events around a burst of launches,
median and range over the rounds), so drift of the box hits all of them alike:

  a  the eval_crop launch (AugConfig.center_crop)
  b  the gpu_augment launch of AugConfig.evaluation on the same store (the 4-tap whole-image
     stretch that was the only evaluation transform before): the yardstick
  c  the FoldedEncoder forward (ResNet-50, ImageNet stem) on the batch that (a) wrote

and, for the validation path, (a) on the same images after an R-capped load (scale 1 on the
shorter side). The ratio a / c decides whether an LDS-staged variant of the kernel is worth
building (the rule: only above 5 %).

  python tools/eval_crop_bench.py [--batch 512] [--size 224] [--rounds 9] [--iters 20]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simclr_pytorch_distributed_amd.data.augment import AugConfig, default_resize, gpu_augment
from simclr_pytorch_distributed_amd.data.datasets import ragged_side_cap

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def imagenet_like_shapes(n, cap, seed):
    """(h, w) with the shorter side in 333..500 and aspect 1..1.5, either orientation, the
    shorter side then capped (aspect kept) as data/datasets.py load_image_folder does."""
    r = np.random.default_rng(seed)
    shapes = []
    for _ in range(n):
        short = int(r.integers(333, 501))
        lng = int(short * r.uniform(1.0, 1.5))
        if short > cap:
            lng, short = max(1, round(lng * cap / short)), cap
        shapes.append((short, lng) if r.random() < 0.7 else (lng, short))
    return shapes


def ragged_store(shapes, seed, dev):
    r = np.random.default_rng(seed)
    sizes = [h * w * 3 for h, w in shapes]
    data = torch.from_numpy(r.integers(0, 256, sum(sizes), dtype=np.uint8))
    offs = torch.tensor(np.cumsum([0] + sizes[:-1]), dtype=torch.int64)
    return data.to(dev), offs.to(dev), torch.tensor(shapes, dtype=torch.int32).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--resize", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model", default="resnet50")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    R = a.resize or default_resize(a.size)
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.ops.linear_probe import FoldedEncoder

    native = ragged_store(imagenet_like_shapes(a.batch, ragged_side_cap(a.size), 0), 1, dev)
    capped = ragged_store(imagenet_like_shapes(a.batch, R, 0), 1, dev)
    idx = torch.from_numpy(np.random.default_rng(2).permutation(a.batch)).to(dev)
    crop = AugConfig.center_crop(a.size, MEAN, STD, R)
    stretch = AugConfig.evaluation(a.size, MEAN, STD)
    torch.manual_seed(0)
    model = SupConResNet(a.model, stem="imagenet").to(dev).to(memory_format=torch.channels_last).eval()
    enc = FoldedEncoder(model.encoder)
    x = gpu_augment(native[0], idx, crop, 0, offs=native[1], hw=native[2])

    def encode():
        with torch.no_grad():
            return enc(x)

    variants = [
        ("a eval_crop native store", lambda: gpu_augment(native[0], idx, crop, 0, offs=native[1], hw=native[2])),
        ("a' eval_crop R-capped store", lambda: gpu_augment(capped[0], idx, crop, 0, offs=capped[1], hw=capped[2])),
        ("b evaluation stretch (4-tap)", lambda: gpu_augment(native[0], idx, stretch, 0, offs=native[1], hw=native[2])),
        (f"c FoldedEncoder {a.model} fwd", encode),
    ]
    mb = sum(int(h) * int(w) * 3 for h, w in native[2].tolist()) / 2 ** 20
    print(f"shape: {a.batch} images -> ({R}, {a.size}); native store {mb:.0f} MiB, shorter side <= "
          f"{ragged_side_cap(a.size)}; {a.rounds} interleaved rounds x {a.iters} launches", flush=True)
    for _, fn in variants:          # warm up every variant
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.iters)
    print(f"{'variant':32s} {'median ms':>10s} {'min':>8s} {'max':>8s}")
    med = {}
    for name, _ in variants:
        t = times[name]
        med[name] = statistics.median(t)
        print(f"{name:32s} {med[name]:10.3f} {min(t):8.3f} {max(t):8.3f}", flush=True)
    names = [n for n, _ in variants]
    ratio = med[names[0]] / med[names[3]]
    print(f"a / c = {100 * ratio:.2f} %  (a' / c = {100 * med[names[1]] / med[names[3]]:.2f} %, "
          f"a / b = {med[names[0]] / med[names[2]]:.2f}x)")
    print("LDS-staged variant: " + ("worth building (a / c above 5 %)" if ratio > 0.05 else
                                    "not built (a / c at or below 5 %: evaluation is encoder-bound)"))


if __name__ == "__main__":
    main()
