"""SimCLR / linear-probe augmentation front-end.

GPU path: ``csrc/kernels/aug.hip`` — the reference's torchvision pipeline
(main_supcon.py:170-179 pretraining; main_ce.py:30-40 linear probe) fused into one
kernel over the HBM-resident uint8 dataset, writing NHWC bf16 (C padded to 8).

CPU path: :func:`augment_reference` — the same pipeline with the *same* counter-based
random draws, in torch (CPU runs, and the oracle the GPU kernel is tested against).
"""
from __future__ import annotations

import math
import dataclasses
from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch
import torch.nn.functional as F

from ..ops import _ext

M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class _Rng:
    def __init__(self, key: int):
        self.key, self.ctr = key, 0

    def uni(self) -> float:
        v = _mix64(self.key ^ _mix64((0x1234567 + self.ctr) & M64))
        self.ctr += 1
        return float(np.float32((v >> 40) * (1.0 / 16777216.0)))


# ---- the LDS plan of the blur kernel: mirror of csrc/include/blur_plan.h -------------------
BLUR_LDS_PER_CU = 160 * 1024
_BLUR_STATIC_LDS = 256
_BLUR_MIN_STRIP = 64
_BLUR_MAX_ROWS = 16


def blur_auto_kernel(size: int) -> int:
    return max(3, (size // 10) | 1)


def _blur_lds_bytes(S, k, rows, strip):
    w = ((k - 1) // 2 + 1 + 3) // 4 * 4
    return 4 * (w + 3 * (rows * min(S, strip + k - 1) + (k + rows - 1) * strip))


def blur_plan(S: int, k: int = 0, rows: int = 0):
    """dict(k, rows, strip, n_strips, lds_bytes) of the blur kernel, or None when the request
    cannot be served (k even or < 3, radius beyond S - 1, no fit in the LDS)."""
    if S < 1 or S > (1 << 15) or k < 0 or k > (1 << 15) or rows < 0 or rows > _BLUR_MAX_ROWS:
        return None
    k = k or blur_auto_kernel(S)
    if k < 3 or k % 2 == 0 or (k - 1) // 2 > S - 1:
        return None
    budget = BLUR_LDS_PER_CU - _BLUR_STATIC_LDS
    if rows == 0:
        fit = [c for c in (4, 2, 1) if _blur_lds_bytes(S, k, c, S) <= BLUR_LDS_PER_CU // 2 - _BLUR_STATIC_LDS] or \
              [c for c in (4, 2, 1) if _blur_lds_bytes(S, k, c, S) <= budget] or [1]
        rows = fit[0]
    n, strip = 1, S
    while _blur_lds_bytes(S, k, rows, strip) > budget:
        n += 1
        strip = (S + n - 1) // n
        if strip < min(S, _BLUR_MIN_STRIP):
            return None
    return dict(k=k, rows=rows, strip=strip, n_strips=(S + strip - 1) // strip,
                lds_bytes=_blur_lds_bytes(S, k, rows, strip))


@dataclass
class AugConfig:
    size: int = 32
    n_views: int = 2
    scale: Sequence[float] = (0.2, 1.0)
    ratio: Sequence[float] = (3 / 4, 4 / 3)
    jitter_p: float = 0.8
    brightness: float = 0.4
    contrast: float = 0.4
    saturation: float = 0.4
    hue: float = 0.1
    gray_p: float = 0.2
    crop: bool = True
    flip: bool = True
    mean: Sequence[float] = (0.4914, 0.4822, 0.4465)
    std: Sequence[float] = (0.2023, 0.1994, 0.2010)
    # RandomApply(GaussianBlur(blur_kernel, sigma ~ U(blur_sigma)), p=blur_p) after grayscale
    # (the SimCLR recipe for ImageNet-sized inputs); off by default
    blur_p: float = 0.0
    blur_kernel: int = 0          # 0 = automatic: 10 % of the side, odd, at least 3
    blur_sigma: Sequence[float] = (0.1, 2.0)
    # evaluation transform Resize(resize) on the shorter side + CenterCrop(size) + normalize
    # (:meth:`center_crop`); 0 = off
    resize: int = 0

    def __post_init__(self):
        if self.resize:
            if self.resize < 0 or not 1 <= self.size <= self.resize <= 32768:
                raise ValueError(f"resize {self.resize} must be in [size, 32768] = [{self.size}, 32768]")
            if self.n_views != 1:
                raise ValueError(f"resize + centre crop makes one view, not n_views = {self.n_views}")
            if self.crop or self.flip or self.jitter_p > 0 or self.gray_p > 0 or self.blur_p > 0:
                raise ValueError("resize + centre crop takes no random stage: crop, flip, jitter_p, gray_p and "
                                 "blur_p must be off")
        if self.blur_p == 0:
            return
        if not 0.0 < self.blur_p <= 1.0:
            raise ValueError(f"blur_p {self.blur_p} must be in [0, 1]")
        k, S = self.blur_k, self.size
        if k < 3 or k % 2 == 0:
            raise ValueError(f"blur_kernel {k} must be odd and >= 3")
        if (k - 1) // 2 > S - 1:
            raise ValueError(f"blur radius {(k - 1) // 2} exceeds size - 1 = {S - 1}: reflect padding is undefined")
        if len(self.blur_sigma) != 2 or not 0.0 < self.blur_sigma[0] <= self.blur_sigma[1]:
            raise ValueError(f"blur_sigma {tuple(self.blur_sigma)} needs 0 < lo <= hi")
        if blur_plan(S, k) is None:
            raise ValueError(f"blur of kernel size {k} at size {S} does not fit the {BLUR_LDS_PER_CU // 1024} KiB LDS")

    @property
    def blur_k(self) -> int:
        """The kernel size in effect."""
        return self.blur_kernel if self.blur_kernel else blur_auto_kernel(self.size)

    @staticmethod
    def simclr(size, mean, std, blur_p=0.0, blur_kernel=0, blur_sigma=(0.1, 2.0)):
        return AugConfig(size=size, mean=mean, std=std, blur_p=blur_p, blur_kernel=blur_kernel,
                         blur_sigma=tuple(blur_sigma))

    @staticmethod
    def linear_train(size, mean, std):
        # main_ce.py:30-35: RandomResizedCrop(32, scale=(0.2, 1)) + flip + normalize
        return AugConfig(size=size, n_views=1, jitter_p=0.0, brightness=0, contrast=0, saturation=0, hue=0,
                         gray_p=0.0, mean=mean, std=std)

    @staticmethod
    def evaluation(size, mean, std):
        # main_ce.py:37-40: ToTensor + normalize
        return AugConfig(size=size, n_views=1, jitter_p=0.0, brightness=0, contrast=0, saturation=0, hue=0,
                         gray_p=0.0, crop=False, flip=False, mean=mean, std=std)

    @staticmethod
    def center_crop(size, mean, std, resize=0):
        """torchvision's evaluation transform Resize(resize) + CenterCrop(size) + normalize;
        ``resize`` 0 = size / 0.875 rounded (256 for 224)."""
        return AugConfig(size=size, n_views=1, jitter_p=0.0, brightness=0, contrast=0, saturation=0, hue=0,
                         gray_p=0.0, crop=False, flip=False, mean=mean, std=std,
                         resize=resize or default_resize(size))


def default_resize(size: int) -> int:
    """The Resize target of a centre crop of ``size``: size / 0.875 rounded (224 -> 256, 32 -> 37)."""
    return (16 * size + 7) // 14


def gpu_augment(data: torch.Tensor, idx: torch.Tensor, cfg: AugConfig, seed, seed_t=None, offs=None,
                hw=None, _blur_rows: int = 0) -> torch.Tensor:
    """``seed_t``: optional int64 device scalar read by the kernel at run time (graph replays).
    ``offs``/``hw``: a ragged native-resolution store (``data`` flat uint8, int64 byte
    offsets, int32 [N, 2] sizes; data/datasets.py load_image_folder).
    ``cfg.blur_p > 0`` runs the kernel with the blur stage. ``_blur_rows`` is not part of the
    interface: rows per barrier round (0 = the plan's choice), for tools/aug_blur_bench.py and the
    tests only; it schedules the stream through LDS and never changes the output.
    ``cfg.resize > 0`` runs the evaluation transform (Resize + CenterCrop + normalize): no draws,
    ``seed`` is unused."""
    m = _ext.require()
    if cfg.resize > 0:
        return m.gpu_eval_crop(data, idx, cfg.size, cfg.resize, list(cfg.mean), list(cfg.std), offs, hw)
    if cfg.blur_p > 0:
        return m.gpu_augment_blur(data, idx, cfg.size, cfg.n_views, int(seed) & ((1 << 63) - 1), list(cfg.mean),
                                  list(cfg.std), cfg.scale[0], cfg.scale[1], cfg.ratio[0], cfg.ratio[1],
                                  cfg.jitter_p, cfg.brightness, cfg.contrast, cfg.saturation, cfg.hue, cfg.gray_p,
                                  cfg.crop, cfg.flip, cfg.blur_p, cfg.blur_k, cfg.blur_sigma[0], cfg.blur_sigma[1],
                                  seed_t, offs, hw, _blur_rows)
    return m.gpu_augment(data, idx, cfg.size, cfg.n_views, int(seed) & ((1 << 63) - 1), list(cfg.mean),
                         list(cfg.std), cfg.scale[0], cfg.scale[1], cfg.ratio[0], cfg.ratio[1], cfg.jitter_p,
                         cfg.brightness, cfg.contrast, cfg.saturation, cfg.hue, cfg.gray_p, cfg.crop, cfg.flip,
                         seed_t, offs, hw)


def _view_params(cfg: AugConfig, H: int, W: int, rng: _Rng):
    f32 = np.float32
    ci, cj, ch, cw = 0.0, 0.0, float(H), float(W)
    if cfg.crop:
        area = f32(H) * f32(W)
        lr0, lr1 = f32(math.log(cfg.ratio[0])), f32(math.log(cfg.ratio[1]))
        found = False
        for _ in range(10):
            target = area * (f32(cfg.scale[0]) + (f32(cfg.scale[1]) - f32(cfg.scale[0])) * f32(rng.uni()))
            ar = f32(math.exp(lr0 + (lr1 - lr0) * f32(rng.uni())))
            w = float(np.rint(f32(math.sqrt(target * ar))))
            h = float(np.rint(f32(math.sqrt(target / ar))))
            if 0 < w <= W and 0 < h <= H:
                ci = math.floor(rng.uni() * (H - h + 1.0))
                cj = math.floor(rng.uni() * (W - w + 1.0))
                ch, cw = h, w
                found = True
                break
        if not found:
            in_ratio = W / H
            if in_ratio < cfg.ratio[0]:
                w, h = W, round(W / cfg.ratio[0])
            elif in_ratio > cfg.ratio[1]:
                h, w = H, round(H * cfg.ratio[1])
            else:
                w, h = W, H
            ci, cj, ch, cw = math.floor((H - h) * 0.5), math.floor((W - w) * 0.5), float(h), float(w)
    flip = cfg.flip and rng.uni() < 0.5
    jitter = rng.uni() < cfg.jitter_p
    fb = 1 + cfg.brightness * (2 * rng.uni() - 1)
    fc = 1 + cfg.contrast * (2 * rng.uni() - 1)
    fs = 1 + cfg.saturation * (2 * rng.uni() - 1)
    fh = cfg.hue * (2 * rng.uni() - 1)
    order = [0, 1, 2, 3]
    for i in range(3, 0, -1):
        j = int(rng.uni() * (i + 1)) % (i + 1)
        order[i], order[j] = order[j], order[i]
    gray = rng.uni() < cfg.gray_p
    if cfg.brightness <= 0 and cfg.contrast <= 0 and cfg.saturation <= 0 and cfg.hue <= 0:
        jitter = False
    # the blur draws come last, so every draw above is the same with the stage on or off
    blur = rng.uni() < cfg.blur_p
    sigma = cfg.blur_sigma[0] + (cfg.blur_sigma[1] - cfg.blur_sigma[0]) * rng.uni()
    return dict(ci=ci, cj=cj, ch=ch, cw=cw, flip=flip, jitter=jitter, fb=fb, fc=fc, fs=fs, fh=fh, order=order,
                gray=gray, blur=blur, sigma=sigma)


def _gaussian_blur(c: torch.Tensor, k: int, sigma: float) -> torch.Tensor:
    """torchvision's tensor gaussian_blur on [3, S, S] fp32: separable, reflect padding."""
    r = (k - 1) // 2
    x = torch.arange(-r, r + 1, dtype=torch.float32)
    w = torch.exp(-0.5 * (x / sigma) ** 2)
    w = w / w.sum()
    S = c.shape[-1]
    pad = F.pad(c.unsqueeze(0), (r, r, 0, 0), mode="reflect")[0]
    c = sum(w[j] * pad[:, :, j:j + S] for j in range(k))
    pad = F.pad(c.unsqueeze(0), (0, 0, r, r), mode="reflect")[0]
    return sum(w[j] * pad[:, j:j + S, :] for j in range(k))


def _grey(img):
    return 0.2989 * img[0] + 0.587 * img[1] + 0.114 * img[2]


def _hue(img, hf):
    r, g, b = img[0], img[1], img[2]
    mx = torch.maximum(r, torch.maximum(g, b))
    mn = torch.minimum(r, torch.minimum(g, b))
    cr = mx - mn
    v = mx
    s = cr / torch.where(mx == 0, torch.ones_like(mx), mx)
    crd = torch.where(cr == 0, torch.ones_like(cr), cr)
    rc, gc, bc = (mx - r) / crd, (mx - g) / crd, (mx - b) / crd
    h = torch.where(mx == r, bc - gc, torch.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h / 6.0 + 1.0
    h = h - torch.floor(h)
    h = h + hf
    h = h - torch.floor(h)
    h6 = h * 6.0
    i = torch.floor(h6)
    f = h6 - i
    p = (v * (1 - s)).clamp(0, 1)
    q = (v * (1 - s * f)).clamp(0, 1)
    t = (v * (1 - s * (1 - f))).clamp(0, 1)
    i = i.long() % 6
    rr = torch.stack([v, q, p, p, t, v])
    gg = torch.stack([t, v, v, q, p, p])
    bb = torch.stack([p, p, t, v, v, q])
    sel = i.unsqueeze(0)
    return torch.stack([rr.gather(0, sel)[0], gg.gather(0, sel)[0], bb.gather(0, sel)[0]])


def resized_hw(H: int, W: int, resize: int):
    """Size of Resize(resize): the shorter side becomes ``resize``, the longer floor(resize·long/short)."""
    lng = (resize * max(H, W)) // min(H, W)
    return (resize, lng) if H <= W else (lng, resize)


def center_crop_offset(d: int) -> int:
    """torchvision's CenterCrop offset int(round(d / 2.0)): half to even."""
    t = d // 2
    return t + 1 if d % 2 and t % 2 else t


def _resize_taps(n_in: int, n_out: int, first: int, count: int) -> torch.Tensor:
    """fp32 [count, n_in] weights of outputs first..first+count-1 of the antialiased bilinear
    resize n_in -> n_out (the triangle filter of F.interpolate(antialias=True)). Window bounds
    and tap offsets are exact integers over 2·n_out, as in aug.hip eval_crop_kernel."""
    sup = max(n_in, n_out)
    i = torch.arange(first, first + count, dtype=torch.int64).unsqueeze(1)
    j = torch.arange(n_in, dtype=torch.int64).unsqueeze(0)
    a = (2 * i + 1) * n_in + n_out
    lo = torch.clamp((a - 2 * sup).div(2 * n_out, rounding_mode="floor"), min=0)
    hi = torch.clamp((a + 2 * sup).div(2 * n_out, rounding_mode="floor"), max=n_in)
    num = 2 * j * n_out + n_out - (2 * i + 1) * n_in
    k = torch.tensor(0.5, dtype=torch.float32) / torch.tensor(float(sup), dtype=torch.float32)
    w = (1.0 - num.abs().float() * k).clamp_(min=0.0)
    w = torch.where((j >= lo) & (j < hi), w, torch.zeros_like(w))
    return w / w.sum(1, keepdim=True)


def _center_crop_reference(data, idx, cfg: AugConfig, offs, hw) -> torch.Tensor:
    """The fp32 CPU twin of aug.hip eval_crop_kernel."""
    B, S, R = idx.shape[0], cfg.size, cfg.resize
    out = torch.zeros(B, S, S, 8)
    mean_t, std_t = torch.tensor(cfg.mean).view(1, 1, 3), torch.tensor(cfg.std).view(1, 1, 3)
    for b in range(B):
        src = int(idx[b])
        if offs is None:
            H, W = data.shape[1], data.shape[2]
            img = data[src].float()
        else:
            H, W = int(hw[src, 0]), int(hw[src, 1])
            o = int(offs[src])
            img = data[o:o + H * W * 3].view(H, W, 3).float()
        oh, ow = resized_hw(H, W, R)
        wy = _resize_taps(H, oh, center_crop_offset(oh - S), S)      # [S, H]
        wx = _resize_taps(W, ow, center_crop_offset(ow - S), S)      # [S, W]
        c = torch.einsum("yh,hwc->ywc", wy, img)
        c = torch.einsum("xw,ywc->yxc", wx, c) / 255.0
        out[b, :, :, :3] = (c - mean_t) / std_t
    return out


def augment_reference(data: torch.Tensor, idx: torch.Tensor, cfg: AugConfig, seed: int, offs=None,
                      hw=None) -> torch.Tensor:
    """CPU torch implementation with identical draws; returns NHWC float [V*B, S, S, 8].
    ``cfg.resize > 0``: the evaluation transform (no draws), [B, S, S, 8]."""
    data = data.cpu()
    idx = idx.cpu()
    if offs is not None:
        offs, hw = offs.cpu(), hw.cpu()
    if cfg.resize > 0:
        return _center_crop_reference(data, idx, cfg, offs, hw)
    B = idx.shape[0]
    S = cfg.size
    seed = int(seed) & ((1 << 63) - 1)
    out = torch.zeros(cfg.n_views * B, S, S, 8)
    oy, ox = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32),
                            indexing="ij")
    for v in range(cfg.n_views):
        for b in range(B):
            src = int(idx[b])
            if offs is None:
                H, W = data.shape[1], data.shape[2]
                img = data[src].float()   # H W 3
            else:
                H, W = int(hw[src, 0]), int(hw[src, 1])
                o = int(offs[src])
                img = data[o:o + H * W * 3].view(H, W, 3).float()
            key = _mix64((seed * 0x100000001B3 + src * 31 + v * 0x9E37 + b) & M64)
            p = _view_params(cfg, H, W, _Rng(key))
            xs = (S - 1 - ox) if p["flip"] else ox
            sy = ((oy + 0.5) * (p["ch"] / S) - 0.5 + p["ci"]).clamp(p["ci"], p["ci"] + p["ch"] - 1)
            sx = ((xs + 0.5) * (p["cw"] / S) - 0.5 + p["cj"]).clamp(p["cj"], p["cj"] + p["cw"] - 1)
            y0, x0 = sy.floor().long(), sx.floor().long()
            y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
            wy, wx = (sy - y0).unsqueeze(-1), (sx - x0).unsqueeze(-1)
            top = img[y0, x0] + (img[y0, x1] - img[y0, x0]) * wx
            bot = img[y1, x0] + (img[y1, x1] - img[y1, x0]) * wx
            c = ((top + (bot - top) * wy) / 255.0).permute(2, 0, 1)   # 3 S S
            if p["jitter"]:
                for op in p["order"]:
                    if op == 0:
                        c = (c * p["fb"]).clamp(0, 1)
                    elif op == 1:
                        mean = _grey(c).mean()
                        c = (p["fc"] * c + (1 - p["fc"]) * mean).clamp(0, 1)
                    elif op == 2:
                        g = _grey(c)
                        c = (p["fs"] * c + (1 - p["fs"]) * g).clamp(0, 1)
                    else:
                        c = _hue(c, p["fh"])
            if p["gray"]:
                c = _grey(c).unsqueeze(0).expand(3, S, S)
            if p["blur"]:
                c = _gaussian_blur(c, cfg.blur_k, p["sigma"])
            mean_t = torch.tensor(cfg.mean).view(3, 1, 1)
            std_t = torch.tensor(cfg.std).view(3, 1, 1)
            c = (c - mean_t) / std_t
            out[v * B + b, :, :, :3] = c.permute(1, 2, 0)
    return out


def augment(data: torch.Tensor, idx: torch.Tensor, cfg: AugConfig, seed: int, offs=None, hw=None) -> torch.Tensor:
    """Dispatch: GPU kernel for GPU tensors, torch reference otherwise (NHWC, C=8)."""
    if data.is_cuda:
        return gpu_augment(data, idx, cfg, seed, offs=offs, hw=hw)
    return augment_reference(data, idx, cfg, seed, offs, hw)


# ---- Mixup / CutMix of an augmented batch (supervised trainer) ------------------------------
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = "none", "mixup", "cutmix"
_MIX_MODE_ID = {MIX_MIXUP: 1, MIX_CUTMIX: 2}       # csrc/include/launchers.h MixMode
# xor-ed into the step seed: the mixing draws share no stream with the augmentation's
_MIX_STREAM = 0x6D69785F64726177


def cutmix_box(lam: float, cy: int, cx: int, S: int):
    """torchvision v2 ``CutMix`` on an S x S image: the box (y0, y1, x0, x1) of half-side
    int(0.5·sqrt(1 − λ)·S) around the centre (cy, cx), clipped to the image, and λ replaced by
    1 − box_area / S²."""
    half = int(0.5 * math.sqrt(1.0 - lam) * S)
    y0, x0 = max(cy - half, 0), max(cx - half, 0)
    y1, x1 = min(cy + half, S), min(cx + half, S)
    return (y0, y1, x0, x1), 1.0 - (y1 - y0) * (x1 - x0) / (S * S)


def mix_draw(opt, seed: int, epoch: int, it: int, rank: int):
    """``(mode, lam, box)`` of one step of one rank: ``mode`` in {none, mixup, cutmix}, one
    λ ~ Beta(α, α) and one box ``(y0, y1, x0, x1)`` for the whole batch (batch mode, as torchvision
    v2 and timm's default). ``opt`` supplies ``mixup`` / ``cutmix`` (the α, 0 = off), ``mix_prob``,
    ``mix_switch_prob`` and ``size``. Host-only and a function of (seed, epoch, it, rank) alone: a
    resumed run draws what the uninterrupted one drew."""
    a_mix, a_cut = float(getattr(opt, "mixup", 0.0)), float(getattr(opt, "cutmix", 0.0))
    none = (MIX_NONE, 1.0, (0, 0, 0, 0))
    if a_mix <= 0 and a_cut <= 0:
        return none
    from ..engine.base import step_seed
    rng = np.random.default_rng(step_seed(seed, epoch, it, rank) ^ _MIX_STREAM)
    # every draw is made whatever the earlier ones decide: one layout of the stream
    u_mix, u_switch = rng.random(), rng.random()
    cut = a_cut > 0 and (a_mix <= 0 or u_switch < float(getattr(opt, "mix_switch_prob", 0.5)))
    alpha = a_cut if cut else a_mix
    lam = float(rng.beta(alpha, alpha))
    S = int(opt.size)
    cy, cx = int(rng.integers(S)), int(rng.integers(S))
    if not u_mix < float(getattr(opt, "mix_prob", 1.0)):
        return none
    if not cut:
        return MIX_MIXUP, lam, (0, 0, 0, 0)
    box, lam = cutmix_box(lam, cy, cx, S)
    return MIX_CUTMIX, lam, box


def mix_views(x: torch.Tensor, mode: str, lam: float, y0: int = 0, y1: int = 0, x0: int = 0, x1: int = 0,
              out=None) -> torch.Tensor:
    """The mixing kernel (csrc/kernels/mix.hip) on a [B, S, S, 8] bf16 batch: image i with image
    (i − 1) mod B, out of place. Mixup: bf16(λ·x[i] + (1 − λ)·x[i−1]); CutMix: x[i−1] inside
    [y0, y1) x [x0, x1), bit for bit."""
    return _ext.require().mix_views(x, _MIX_MODE_ID[mode], float(lam), y0, y1, x0, x1, out)


def mix_reference(x: torch.Tensor, mode: str, lam: float, box=(0, 0, 0, 0), layout: str = "nchw") -> torch.Tensor:
    """The fp32 torch twin of :func:`mix_views` (torch backend, CPU, ``--gpu_aug 0``): ``x`` is
    [B, C, H, W] (``layout="nchw"``) or [B, H, W, C]; λ and 1 − λ are taken in fp32 as the kernel
    takes them, and the result has x's dtype (one rounding)."""
    xr = x.roll(1, 0)
    if mode == MIX_CUTMIX:
        y0, y1, x0, x1 = box
        out = x.clone()
        if layout == "nchw":
            out[:, :, y0:y1, x0:x1] = xr[:, :, y0:y1, x0:x1]
        else:
            out[:, y0:y1, x0:x1, :] = xr[:, y0:y1, x0:x1, :]
        return out
    if mode != MIX_MIXUP:
        raise ValueError(f"mix mode {mode!r}")
    w0 = np.float32(lam)
    w1 = np.float32(1.0) - w0
    return (float(w0) * x.float() + float(w1) * xr.float()).to(x.dtype)


def nhwc8_to_nchw(x: torch.Tensor) -> torch.Tensor:
    """NHWC [.., 8] -> NCHW float [.., 3, H, W] for the torch backend."""
    return x[..., :3].permute(0, 3, 1, 2).float().contiguous()


class SimCLRAugment:
    """Per-sample callable form of the SimCLR augmentation (reference main_supcon.py:170-179):
    a uint8 HWC image tensor -> normalized float CHW [3, S, S], with the same draws as the
    batched kernels. Each call advances an internal counter, so repeated calls on one image
    give independent views (use with :class:`TwoCropTransform`)."""

    def __init__(self, cfg: AugConfig, seed: int = 0):
        self.cfg = dataclasses.replace(cfg, n_views=1)
        self.seed = int(seed)
        self._calls = 0

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3, "uint8 HWC image"
        self._calls += 1
        out = augment_reference(img.unsqueeze(0), torch.zeros(1, dtype=torch.long), self.cfg,
                                _mix64((self.seed * 0x9E3779B97F4A7C15 + self._calls) & M64))
        return out[0, :, :, :3].permute(2, 0, 1).contiguous()


class TwoCropTransform:
    """Two independently augmented views of one sample (reference util.py:10-16). The
    training engines draw both views of a whole batch in one GPU launch instead
    (:func:`gpu_augment` with ``n_views=2``); this wrapper serves per-sample pipelines."""

    def __init__(self, transform):
        self.transform = transform

    def __call__(self, x):
        return [self.transform(x), self.transform(x)]
