"""fp64 numpy oracle of the evaluation transform Resize(R) + CenterCrop(S) + normalize
(data/augment.py AugConfig.center_crop, csrc/kernels/aug.hip eval_crop_kernel), written from
the definition and independent of both implementations.

For a source H x W, the shorter side becomes R and the longer floor(R * long / short). Per axis
n_in -> n_out: scale = n_in / n_out, support = max(scale, 1), centre c = scale (i + 0.5), taps
j in [max(0, floor(c - support + 0.5)), min(n_in, floor(c + support + 0.5))) with weight
max(0, 1 - |j - c + 0.5| / support) divided by the window's sum (the triangle filter of
``F.interpolate(mode="bilinear", antialias=True)``). The window bounds are worked out in exact
integer arithmetic; tests/test_evalcrop_oracle.py checks them against the floating-point
definition and the resized image against torch in float64. The crop offset is torchvision's
``int(round((o - S) / 2.0))`` (half to even). No uint8 intermediate image.

A case is a list of runs; a run is one launch: a store (dense or ragged), ``idx`` and a config.

``EPS_CROP_REF`` is the measured worst deviation of the fp32 ``augment_reference`` from this
oracle over all cases, in pre-normalise colour units ([0, 1]); tests/test_evalcrop_oracle.py
measures and asserts it, and tests/test_gpu_evalcrop.py derives the GPU floor from it.
"""
from __future__ import annotations

import os

import numpy as np

import aug_oracle as O
from simclr_pytorch_distributed_amd.data import augment as A

MEAN, STD = O.MEAN, O.STD

# worst |augment_reference - oracle| over CASES, colour units in [0, 1] (measured; asserted in
# tests/test_evalcrop_oracle.py::test_eps_crop_ref_is_the_measured_worst)
EPS_CROP_REF = 2.2e-7


def resized_hw(H: int, W: int, R: int):
    lng = (R * max(H, W)) // min(H, W)
    return (R, lng) if H <= W else (lng, R)


def window(n_in: int, n_out: int, i: int):
    """[lo, hi) of output i, in exact integers: with sup = max(n_in, n_out) (support = sup / n_out),
    floor(c -+ support + 0.5) = floor(((2i + 1) n_in -+ 2 sup + n_out) / (2 n_out))."""
    sup = max(n_in, n_out)
    a = (2 * i + 1) * n_in + n_out
    return max(0, (a - 2 * sup) // (2 * n_out)), min(n_in, (a + 2 * sup) // (2 * n_out))


def axis_weights(n_in: int, n_out: int) -> np.ndarray:
    """float64 [n_out, n_in] resize matrix of one axis."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        lo, hi = window(n_in, n_out, i)
        c = scale * (i + 0.5)
        j = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) / support))
        m[i, lo:hi] = w / w.sum()
    return m


def resize(img: np.ndarray, R: int) -> np.ndarray:
    """uint8 [H, W, 3] -> float64 [oh, ow, 3] on the 0-255 scale."""
    H, W = img.shape[:2]
    oh, ow = resized_hw(H, W, R)
    rows = np.einsum("yh,hwc->ywc", axis_weights(H, oh), img.astype(np.float64))
    return np.einsum("xw,ywc->yxc", axis_weights(W, ow), rows)


def crop_offset(d: int) -> int:
    """int(round(d / 2.0)), half to even, in integers."""
    if d % 2 == 0:
        return d // 2
    return (d - 1) // 2 if ((d - 1) // 2) % 2 == 0 else (d + 1) // 2


def transform(img: np.ndarray, R: int, S: int):
    """(colour [S, S, 3] in [0, 1], (top, left)) float64."""
    r = resize(img, R)
    top, left = crop_offset(r.shape[0] - S), crop_offset(r.shape[1] - S)
    return r[top:top + S, left:left + S] / 255.0, (top, left)


# ---------------------------------------------------------------- cases ------------------------

def _run(shapes, R, S, seed, idx=None, dense=None):
    cfg = A.AugConfig.center_crop(S, MEAN, STD, resize=R)
    if dense is not None:
        return O._case("", cfg, 0, idx if idx is not None else list(range(dense[0])), O._dense(*dense, seed))
    return O._case("", cfg, 0, idx if idx is not None else list(range(len(shapes))), ragged=O._ragged(shapes, seed))


LANDSCAPE, PORTRAIT = (37, 53), (53, 37)
MIX = [LANDSCAPE, PORTRAIT, (16, 23), (9, 12), (200, 300), (8, 200), (32, 32)]
MIX_IDX = [4, 0, 6, 2, 2, 5, 1, 3, 0, 4, 6, 1, 5, 3, 2, 0]
IMAGENET = [(500, 375), (375, 500), (256, 341)]

_BUILDERS = {
    "down_landscape": lambda: [_run([LANDSCAPE], 16, 14, 21)],
    "down_portrait": lambda: [_run([PORTRAIT], 16, 14, 22)],
    "odd_offsets": lambda: [_run([LANDSCAPE], 16, 13, 23), _run([LANDSCAPE], 16, 15, 23), _run([LANDSCAPE], 17, 12, 23)],
    "identity": lambda: [_run([(16, 23)], 16, 16, 24)],
    "upsample": lambda: [_run([(9, 12)], 16, 16, 25)],
    "extreme": lambda: [_run([(200, 300), (8, 200)], 16, 16, 26)],
    "dense": lambda: [_run(None, 37, 32, 27, idx=[3, 0, 4, 1, 2], dense=(5, 32, 32))],
    "ragged_mix": lambda: [_run(MIX, 16, 14, 28, idx=MIX_IDX)],
    "imagenet": lambda: [_run(IMAGENET, 256, 224, 29)],
}

CASES = list(_BUILDERS)
_cache = {}


def get_case(name):
    """The runs of a case with the oracle attached (``norm`` [B, S, S, 3] float64, ``offsets``
    per row); computed once per process, never modified."""
    if name not in _cache:
        runs = _BUILDERS[name]()
        for run in runs:
            cfg = run["cfg"]
            res = [transform(O.image(run, int(s)), cfg.resize, cfg.size) for s in run["idx"]]
            run["colour"] = np.stack([c for c, _ in res])
            run["norm"] = (run["colour"] - np.asarray(cfg.mean)) / np.asarray(cfg.std)
            run["offsets"] = [o for _, o in res]
        _cache[name] = runs
    return _cache[name]


# ---------------------------------------------------------------- a small ImageFolder ----------

MEAN_S, STD_S = "(0.5,0.45,0.4)", "(0.25,0.2,0.22)"


def make_image_folder(root, n_train=8, n_val=4, seed=0):
    """3 classes of PNGs with sides 40..70 px and a class-dependent colour; (train, val) folders."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    base = [(200, 60, 60), (60, 200, 60), (60, 60, 200)]
    for split, n in (("train", n_train), ("val", n_val)):
        for c, col in enumerate(base):
            d = os.path.join(root, split, f"class{c}")
            os.makedirs(d)
            for i in range(n):
                h, w = (int(v) for v in rng.integers(40, 71, 2))
                img = np.clip(np.asarray(col) + rng.normal(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(d, f"{i}.png"))
    return os.path.join(root, "train"), os.path.join(root, "val")
