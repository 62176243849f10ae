"""fp64 numpy oracle of the augmentation pixel pipeline, written from the definitions of the
torchvision transforms the project reproduces (RandomResizedCrop -> RandomHorizontalFlip ->
RandomApply(ColorJitter) -> RandomGrayscale -> ToTensor -> Normalize), given EXPLICIT view
parameters (crop box, flip, the four factors, op order, gray).

Only the random draws come from the implementation (``augment._Rng`` / ``_view_params`` and the
per-view key): they are the specification of the counter hash, nothing independent exists for
them. :func:`redraw_crop` recomputes the crop draw in fp64 from the same uniform stream to find
the views whose float32 draw sits on a rounding edge (``fragile``), and checks the box of every
other view.

``EPS_REF`` is the measured worst deviation of the fp32 torch ``augment_reference`` from this
oracle over ``CASES`` in pre-normalise colour units (tests/test_augment_oracle.py measures and
asserts it); the GPU acceptance floor is derived from it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from simclr_pytorch_distributed_amd.data import augment as A

# worst |augment_reference - oracle| over CASES, colour units in [0, 1] (measured; asserted in
# tests/test_augment_oracle.py::test_reference_matches_oracle)
EPS_REF = 1.7e-6

MEAN = (0.4914, 0.4822, 0.4465)
STD = (0.2023, 0.1994, 0.2010)
GREY_W = np.array([0.2989, 0.587, 0.114])


# ---------------------------------------------------------------- pixel pipeline (fp64) ------

def _axis(n_in: int, S: int):
    """bilinear source taps of one axis, align_corners=False, no antialias."""
    src = (np.arange(S, dtype=np.float64) + 0.5) * (n_in / S) - 0.5
    src = np.clip(src, 0.0, n_in - 1.0)
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def resized_crop(img_u8: np.ndarray, ci: int, cj: int, ch: int, cw: int, S: int) -> np.ndarray:
    """[H, W, 3] uint8 -> [S, S, 3] float64 in [0, 1]: crop the box, then resize it."""
    crop = img_u8[ci:ci + ch, cj:cj + cw].astype(np.float64) / 255.0
    assert crop.shape[:2] == (ch, cw), "box outside the image"
    y0, y1, ly = _axis(ch, S)
    x0, x1, lx = _axis(cw, S)
    rows = crop[y0] * (1.0 - ly)[:, None, None] + crop[y1] * ly[:, None, None]
    return rows[:, x0] * (1.0 - lx)[None, :, None] + rows[:, x1] * lx[None, :, None]


def grey(c: np.ndarray) -> np.ndarray:
    return c @ GREY_W


def _blend(a, b, f):
    return np.clip(f * a + (1.0 - f) * b, 0.0, 1.0)


def brightness(c, f):
    return _blend(c, 0.0, f)


def contrast(c, f):
    return _blend(c, grey(c).mean(), f)


def saturation(c, f):
    return _blend(c, grey(c)[..., None], f)


def hue(c, hf):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(-1), c.min(-1)
    eq = mx == mn
    cr = mx - mn
    s = cr / np.where(eq, 1.0, mx)
    div = np.where(eq, 1.0, cr)
    rc, gc, bc = (mx - r) / div, (mx - g) / div, (mx - b) / div
    is_r = mx == r
    is_g = (mx == g) & ~is_r
    is_b = ~is_g & ~is_r
    h = is_r * (bc - gc) + is_g * (2.0 + rc - bc) + is_b * (4.0 + gc - rc)
    h = np.mod(h / 6.0 + 1.0, 1.0)
    h = np.mod(h + hf, 1.0)
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.astype(np.int64) % 6
    v = mx
    p = np.clip(v * (1.0 - s), 0.0, 1.0)
    q = np.clip(v * (1.0 - s * f), 0.0, 1.0)
    t = np.clip(v * (1.0 - s * (1.0 - f)), 0.0, 1.0)
    table = np.stack([np.stack([v, q, p, p, t, v]),      # red   by sector
                      np.stack([t, v, v, q, p, p]),      # green
                      np.stack([p, p, t, v, v, q])])     # blue     [3, 6, ...]
    out = np.take_along_axis(table, i[None, None], axis=1)[:, 0]
    return np.moveaxis(out, 0, -1)


_OPS = (brightness, contrast, saturation, hue)


def oracle_view(img_u8, S, box, flip, jitter, factors, order, gray, mean=MEAN, std=STD):
    """One view -> ([S, S, 3] colour in [0, 1], [S, S, 3] normalised), both float64."""
    c = resized_crop(img_u8, *box, S)
    if flip:
        c = c[:, ::-1]
    if jitter:
        for op in order:
            c = _OPS[op](c, factors[op])
    if gray:
        c = np.repeat(grey(c)[..., None], 3, axis=-1)
    return c, (c - np.asarray(mean)) / np.asarray(std)


# ---------------------------------------------------------------- draws ------------------------

def view_key(seed: int, src: int, v: int, b: int) -> int:
    seed = int(seed) & ((1 << 63) - 1)
    return A._mix64((seed * 0x100000001B3 + src * 31 + v * 0x9E37 + b) & A.M64)


def _near_half(x, eps=1e-3):
    return abs((x - 0.5) - round(x - 0.5)) < eps


def _near_int(x, eps=1e-3):
    return abs(x - round(x)) < eps


def redraw_crop(cfg, H: int, W: int, key: int):
    """The RandomResizedCrop draw recomputed in fp64 from the view's uniform stream.
    Returns (box, fragile, fallback, tries). ``fragile``: some rint argument within 1e-3 of a
    half-integer, or some floor argument within 1e-3 of an integer, so a float32 evaluation
    may round the other way."""
    if not cfg.crop:
        return (0, 0, H, W), False, False, 0
    rng = A._Rng(key)
    fragile = False
    lr0, lr1 = math.log(cfg.ratio[0]), math.log(cfg.ratio[1])
    for t in range(10):
        target = H * W * (cfg.scale[0] + (cfg.scale[1] - cfg.scale[0]) * rng.uni())
        ar = math.exp(lr0 + (lr1 - lr0) * rng.uni())
        wa, ha = math.sqrt(target * ar), math.sqrt(target / ar)
        fragile |= _near_half(wa) or _near_half(ha)
        w, h = round(wa), round(ha)
        if 0 < w <= W and 0 < h <= H:
            ya, xa = rng.uni() * (H - h + 1), rng.uni() * (W - w + 1)
            fragile |= _near_int(ya) or _near_int(xa)
            return (math.floor(ya), math.floor(xa), h, w), fragile, False, t + 1
    in_ratio = W / H
    if in_ratio < cfg.ratio[0]:
        fragile |= _near_half(W / cfg.ratio[0])
        w, h = W, round(W / cfg.ratio[0])
    elif in_ratio > cfg.ratio[1]:
        fragile |= _near_half(H * cfg.ratio[1])
        h, w = H, round(H * cfg.ratio[1])
    else:
        w, h = W, H
    fragile |= min(abs(in_ratio / cfg.ratio[0] - 1.0), abs(in_ratio / cfg.ratio[1] - 1.0)) < 1e-6
    return ((H - h) // 2, (W - w) // 2, h, w), fragile, True, 10


def views(case):
    """Per output row (view-major: row v*B + b <-> idx[b]): dict(img, params, box, fragile,
    fallback, tries). The box of a non-fragile view must equal the fp64 recomputation."""
    cfg, idx = case["cfg"], case["idx"]
    B = len(idx)
    rows = []
    for v in range(cfg.n_views):
        for b in range(B):
            src = int(idx[b])
            img = image(case, src)
            H, W = img.shape[:2]
            key = view_key(case["seed"], src, v, b)
            p = A._view_params(cfg, H, W, A._Rng(key))
            box, fragile, fallback, tries = redraw_crop(cfg, H, W, key)
            pbox = (int(p["ci"]), int(p["cj"]), int(p["ch"]), int(p["cw"]))
            if not fragile:
                assert pbox == box, (case["name"], v, b, pbox, box)
            rows.append(dict(img=img, p=p, box=pbox, fragile=fragile, fallback=fallback, tries=tries))
    return rows


def oracle_batch(case, rows=None):
    """([V*B, S, S, 3] colour, [V*B, S, S, 3] normalised) float64, rows as ``views``."""
    cfg = case["cfg"]
    rows = rows if rows is not None else views(case)
    col, nrm = [], []
    for r in rows:
        p = r["p"]
        c, n = oracle_view(r["img"], cfg.size, r["box"], p["flip"], p["jitter"],
                           (p["fb"], p["fc"], p["fs"], p["fh"]), p["order"], p["gray"], cfg.mean, cfg.std)
        col.append(c)
        nrm.append(n)
    return np.stack(col), np.stack(nrm)


# ---------------------------------------------------------------- cases ------------------------

def image(case, src: int) -> np.ndarray:
    if case["hw"] is None:
        return case["data"][src].numpy()
    h, w = (int(x) for x in case["hw"][src])
    o = int(case["offs"][src])
    return case["data"][o:o + h * w * 3].view(h, w, 3).numpy()


def _cfg(size, n_views=2, **kw):
    base = dict(jitter_p=0.0, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0, gray_p=0.0, crop=False,
                flip=False, mean=MEAN, std=STD)
    base.update(kw)
    return A.AugConfig(size=size, n_views=n_views, **base)


def _dense(n, H, W, seed):
    r = np.random.default_rng(seed)
    return torch.from_numpy(r.integers(0, 256, (n, H, W, 3), dtype=np.uint8))


def _ragged(shapes, seed):
    r = np.random.default_rng(seed)
    imgs = [torch.from_numpy(r.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in shapes]
    data = torch.cat([i.reshape(-1) for i in imgs])
    offs = torch.tensor(np.cumsum([0] + [h * w * 3 for h, w in shapes[:-1]]), dtype=torch.int64)
    return data, offs, torch.tensor(shapes, dtype=torch.int32)


def palette_images(n_random=2, side=16, seed=5):
    """Image 0: black, white, greys, the six primaries/secondaries, pixels with two equal
    maxima, values that clamp under brightness 1.4, then random pixels. Others: random."""
    pal = [(0, 0, 0), (255, 255, 255), (1, 1, 1), (64, 64, 64), (128, 128, 128), (200, 200, 200), (254, 254, 254),
           (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
           (200, 200, 10), (10, 200, 200), (200, 10, 200), (90, 90, 30), (30, 90, 90), (90, 30, 90),   # two maxima
           (200, 200, 199), (199, 200, 200), (200, 199, 200), (100, 100, 101),                       # near-grey
           (190, 230, 250), (183, 20, 240), (250, 185, 5), (182, 182, 183), (255, 128, 0), (0, 128, 255),  # clamp
           (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 254, 253), (3, 2, 1)]
    data = _dense(1 + n_random, side, side, seed)
    flat = data[0].view(-1, 3)
    flat[:len(pal)] = torch.tensor(pal, dtype=torch.uint8)
    return data


def _case(name, cfg, seed, idx, data=None, ragged=None):
    if ragged is not None:
        data, offs, hw = ragged
    else:
        offs = hw = None
    return dict(name=name, cfg=cfg, seed=seed, idx=torch.tensor(idx, dtype=torch.int64), data=data, offs=offs, hw=hw)


FULL = dict(jitter_p=1.0, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1)
SIMCLR = dict(jitter_p=0.8, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, gray_p=0.2, crop=True, flip=True)
RAGGED_CROP = [(48, 64), (33, 33), (90, 40), (40, 90), (57, 71)]
FALLBACK = [(40, 90), (90, 40), (33, 33)]

# seeds marked "chosen" were picked on the CPU so that the condition the tests assert before
# any GPU call holds (order coverage, both flip outcomes, fragile share, fallback reached)
_BUILDERS = {
    "identity_v1": lambda: _case("identity_v1", _cfg(8, 1), 3, [3, 0, 3, 6, 0], _dense(7, 8, 8, 1)),
    "identity_v2": lambda: _case("identity_v2", _cfg(8, 2), 3, [3, 0, 3, 6, 0], _dense(7, 8, 8, 1)),
    "identity_v3": lambda: _case("identity_v3", _cfg(8, 3), 3, [3, 0, 3, 6, 0], _dense(7, 8, 8, 1)),
    "resize_32_24": lambda: _case("resize_32_24", _cfg(24), 4, [2, 0, 3], _dense(4, 32, 32, 2)),
    "resize_32_7": lambda: _case("resize_32_7", _cfg(7), 4, [2, 0, 3], _dense(4, 32, 32, 2)),
    "resize_32_1": lambda: _case("resize_32_1", _cfg(1), 4, [2, 0, 3], _dense(4, 32, 32, 2)),
    "ragged_20x28_32": lambda: _case("ragged_20x28_32", _cfg(32), 5, [1, 0, 1], ragged=_ragged([(20, 28), (28, 20)], 3)),
    "ragged_tiny_8": lambda: _case("ragged_tiny_8", _cfg(8), 5, [0, 1, 2, 1],
                                   ragged=_ragged([(1, 1), (1, 9), (9, 1)], 4)),
    "flip_only": lambda: _case("flip_only", _cfg(16, flip=True), 6, [0, 1, 2, 3, 4, 5, 6, 7], _dense(8, 16, 16, 5)),
    "jitter_brightness": lambda: _case("jitter_brightness", _cfg(16, jitter_p=1.0, brightness=0.4), 7,
                                       [0, 1, 0, 2, 0, 0, 1, 0], palette_images()),
    "jitter_contrast": lambda: _case("jitter_contrast", _cfg(16, jitter_p=1.0, contrast=0.4), 7,
                                     [0, 1, 0, 2, 0, 0, 1, 0], palette_images()),
    "jitter_saturation": lambda: _case("jitter_saturation", _cfg(16, jitter_p=1.0, saturation=0.4), 7,
                                       [0, 1, 0, 2, 0, 0, 1, 0], palette_images()),
    "jitter_hue": lambda: _case("jitter_hue", _cfg(16, jitter_p=1.0, hue=0.1), 7, [0, 1, 0, 2, 0, 0, 1, 0],
                                palette_images()),
    "jitter_hue_wide": lambda: _case("jitter_hue_wide", _cfg(16, jitter_p=1.0, hue=0.5), 7,
                                     [0, 1, 0, 2, 0, 0, 1, 0], palette_images()),
    # chosen: the 64 views cover all 24 op orders
    "jitter_full": lambda: _case("jitter_full", _cfg(16, **FULL), JITTER_FULL_SEED,
                                 [i % 3 for i in range(32)], palette_images()),
    "gray_only": lambda: _case("gray_only", _cfg(16, gray_p=1.0), 8, [0, 1, 2, 0], palette_images()),
    "gray_jitter": lambda: _case("gray_jitter", _cfg(16, gray_p=1.0, **FULL), 8, [0, 1, 2, 0, 0, 1, 2, 0],
                                 palette_images()),
    # chosen: fragile views <= 5 % of the batch
    "crop_standard": lambda: _case("crop_standard", _cfg(32, **SIMCLR), CROP_SEED, list(range(32)),
                                   _dense(32, 32, 32, 6)),
    "crop_to_24": lambda: _case("crop_to_24", _cfg(24, crop=True, flip=True), CROP_SEED, list(range(16)),
                                _dense(16, 32, 32, 6)),
    "crop_high_scale": lambda: _case("crop_high_scale", _cfg(32, crop=True, flip=True, scale=(0.9, 1.0)), CROP_SEED,
                                     list(range(32)), _dense(32, 32, 32, 6)),
    "crop_ragged": lambda: _case("crop_ragged", _cfg(32, **SIMCLR), CROP_SEED, [i % 5 for i in range(20)],
                                 ragged=_ragged(RAGGED_CROP, 7)),
    # chosen: some 33x33 view runs out of tries
    "crop_fallback": lambda: _case("crop_fallback", _cfg(16, crop=True, scale=(1.0, 1.0)), FALLBACK_SEED,
                                   [0, 1, 2, 2, 1, 0, 2, 2], ragged=_ragged(FALLBACK, 8)),
}

JITTER_FULL_SEED = 12
CROP_SEED = 1
FALLBACK_SEED = 2

CASES = list(_BUILDERS)
_cache = {}


def get_case(name):
    """Case inputs with the oracle attached (computed once per process, never modified)."""
    if name not in _cache:
        case = _BUILDERS[name]()
        case["rows"] = views(case)
        case["colour"], case["norm"] = oracle_batch(case, case["rows"])
        _cache[name] = case
    return _cache[name]
