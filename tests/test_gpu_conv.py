"""Implicit-GEMM MFMA convolution kernels vs fp32 torch convolution (GPU)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, H, W, C, K, R, stride, pad)
SHAPES = [
    (4, 8, 8, 64, 64, 1, 1, 0),
    (3, 8, 8, 64, 256, 1, 1, 0),
    (2, 9, 7, 128, 64, 3, 1, 1),     # ragged spatial, M tail
    (4, 8, 8, 64, 128, 3, 2, 1),     # strided 3x3
    (4, 8, 8, 256, 512, 1, 2, 0),    # strided 1x1 shortcut
    (8, 8, 8, 8, 64, 3, 1, 1),       # stem (C padded to 8)
    (2, 4, 4, 512, 512, 3, 1, 1),    # layer4 shape
    (8, 16, 16, 128, 256, 3, 1, 1),  # several 256-row tiles, 18 K-tiles (ping-pong ring wraps)
    (4, 16, 16, 192, 320, 1, 1, 0),  # 3 K-tiles (shortest ping-pong), ragged N vs 128/256
]


def _mk(N, H, W, C, K, R, seed=0, dev="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g).to(dev).bfloat16()
    w = (torch.randn(K, C, R, R, generator=g) / (C * R * R) ** 0.5).to(dev).bfloat16()
    return x, w


def _rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-6)).item()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, 6])
def test_conv_fwd(gpu, shape, cfg):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    ref = F.conv2d(x.float(), w.float(), stride=st, padding=pad)                  # NCHW fp32
    xh = x.permute(0, 2, 3, 1).contiguous()
    wh = w.permute(0, 2, 3, 1).contiguous()
    y, slab = m.conv_fwd(xh, wh, st, pad, True, cfg)
    yr = y.permute(0, 3, 1, 2).float()
    assert _rel(yr, ref) < 1e-2
    # stats come from the fp32 accumulators (before bf16 rounding of the stored y)
    sums = m.bn_stats_reduce(slab)
    yf = ref.permute(0, 2, 3, 1).reshape(-1, K).double()
    assert torch.allclose(sums[0], yf.sum(0), rtol=1e-3, atol=1e-2)
    assert torch.allclose(sums[1], (yf * yf).sum(0), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, 6])
def test_conv_dgrad(gpu, shape, cfg):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    xf = x.float().requires_grad_(True)
    out = F.conv2d(xf, w.float(), stride=st, padding=pad)
    dy = torch.randn_like(out).bfloat16()
    (dx_ref,) = torch.autograd.grad(out, xf, dy.float())
    wt = w.permute(1, 2, 3, 0).contiguous()            # [C][R][S][K]
    dx = m.conv_dgrad(dy.permute(0, 2, 3, 1).contiguous(), wt, H, W, st, pad, cfg)
    assert _rel(dx.permute(0, 3, 1, 2), dx_ref) < 1e-2


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_conv_wgrad(gpu, shape, cfg):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, stride=st, padding=pad)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    for splits in (1, 3):
        dw = m.conv_wgrad(dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous(), R, R, st, pad,
                          splits, cfg)
        assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3


@pytest.mark.parametrize("shape", [(4, 32, 32, 64, 64), (3, 16, 16, 128, 64), (2, 16, 16, 64, 128),
                                   (5, 8, 8, 128, 128), (6, 4, 4, 64, 192), (4, 4, 4, 256, 64)])
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad3x3_tap_reuse(gpu, shape, splits):
    """Tap-reuse 3x3 wgrad (cfg 9, wgrad3x3.hip) vs fp32 torch: images of width 32/16/8/4
    (a 32-pixel step spans 1/2/4/8 rows, crossing image boundaries at width 4 and 8),
    direct (1 split), split-K, and auto split; plus accumulation into a KRSC sink."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape[0], shape[1], shape[3], shape[4]
    x, w = _mk(N, H, H, C, K, 3)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, padding=1)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    dw = m.conv_wgrad(dyh, xh, 3, 3, 1, 1, splits, 9)
    assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
    sink = torch.full((K, 3, 3, C), 0.25, device=gpu)
    m.conv_wgrad(dyh, xh, 3, 3, 1, 1, splits, 9, sink, True)
    assert _rel(sink - 0.25, dw.float()) < 1e-5
    # auto dispatch picks the same kernel for these shapes
    dw2 = m.conv_wgrad(dyh, xh, 3, 3, 1, 1, splits, -1) if splits == 0 else dw
    assert torch.equal(dw2, dw)


@pytest.mark.parametrize("shape", [(4, 16, 256, 128), (2, 8, 512, 256), (8, 4, 128, 512), (3, 8, 384, 128),
                                   (6, 4, 256, 128), (16, 16, 256, 256),
                                   (4, 16, 64, 256), (4, 16, 256, 64), (2, 16, 64, 64), (3, 8, 64, 128),
                                   (3, 8, 128, 64)])
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad1x1_stream(gpu, shape, splits):
    """Stride-1 1x1 wgrad kernels (cfg 10, wgrad1x1.hip) vs fp32 torch: 128- and 256-wide
    column tiles, direct / split-K / auto split, accumulation into a sink, auto dispatch.
    A 64-channel side (the last five shapes) runs on the opt-in pixel-pair view: two pixels'
    64 channels per 128-wide row, the diagonal blocks stored as two slab slices per split."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 1)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    prev = m.wgrad1x1_pairs_set(1)   # the pixel-pair view is opt-in
    try:
        _wgrad1x1_checks(m, dyh, xh, dw_ref, splits, K, C, gpu)
    finally:
        m.wgrad1x1_pairs_set(prev)


def _wgrad1x1_checks(m, dyh, xh, dw_ref, splits, K, C, gpu):
    dw = m.conv_wgrad(dyh, xh, 1, 1, 1, 0, splits, 10)
    assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
    sink = torch.full((K, 1, 1, C), 0.25, device=gpu)
    m.conv_wgrad(dyh, xh, 1, 1, 1, 0, splits, 10, sink, True)
    assert _rel(sink - 0.25, dw.float()) < 1e-5
    if splits == 0:
        assert torch.equal(m.conv_wgrad(dyh, xh, 1, 1, 1, 0, 0, -1), dw)


@pytest.mark.parametrize("shape", [(4, 7, 64, 128), (3, 14, 128, 64), (2, 28, 64, 64), (2, 56, 64, 64),
                                   (3, 12, 64, 64), (2, 40, 128, 64)])
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad3x3_padded_width(gpu, shape, splits):
    """Stride-1 tap-reuse 3x3 wgrad for widths that are not a power of two
    (wgrad3x3_pad_kernel: 32 slots per step as rows padded to 8/16/32 slots, or half rows of
    a 64-slot row — the 224x224 config's 56/28/14/7 and others) vs fp32 torch: direct,
    split-K, auto split, accumulation into a sink, auto dispatch."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 3)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, padding=1)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    dw = m.conv_wgrad(dyh, xh, 3, 3, 1, 1, splits, 9)
    assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
    sink = torch.full((K, 3, 3, C), 0.25, device=gpu)
    m.conv_wgrad(dyh, xh, 3, 3, 1, 1, splits, 9, sink, True)
    assert _rel(sink - 0.25, dw.float()) < 1e-5
    if splits == 0:
        assert torch.equal(m.conv_wgrad(dyh, xh, 3, 3, 1, 1, 0, -1), dw)


@pytest.mark.parametrize("shape", [(4, 64, 64, 64), (4, 32, 128, 64), (3, 16, 64, 128), (4, 8, 128, 192),
                                   (4, 14, 64, 128), (3, 28, 128, 64), (2, 56, 64, 64), (3, 24, 64, 64)])
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad3x3_stride2(gpu, shape, splits):
    """Stride-2 tap-reuse 3x3 wgrad (wgrad3x3_s2_kernel: de-interleaved x window; the first
    3x3 of layers 2-4, reference networks/resnet_big.py:45) vs fp32 torch: output widths
    32 / 16 / 8 / 4 (a 32-pixel step is 1 / 2 / 4 / 8 output rows, crossing images at 8 and 4)
    and 7 / 14 / 28 / 12 on padded rows of 8 / 16 / 32 / 16 slots (the 224x224 config),
    direct / split-K / auto split, accumulation into a sink, auto dispatch."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 3)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, stride=2, padding=1)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    dw = m.conv_wgrad(dyh, xh, 3, 3, 2, 1, splits, 9)
    assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
    sink = torch.full((K, 3, 3, C), 0.25, device=gpu)
    m.conv_wgrad(dyh, xh, 3, 3, 2, 1, splits, 9, sink, True)
    assert _rel(sink - 0.25, dw.float()) < 1e-5
    if splits == 0:
        assert torch.equal(m.conv_wgrad(dyh, xh, 3, 3, 2, 1, 0, -1), dw)


@pytest.mark.parametrize("shape", [(4, 32, 256, 512), (8, 16, 512, 256), (16, 8, 256, 128), (4, 8, 128, 256),
                                   (32, 14, 128, 256), (8, 28, 128, 128), (4, 56, 256, 128), (2, 24, 128, 128)])
@pytest.mark.parametrize("splits", [1, 3, 0])
def test_wgrad1x1_strided(gpu, shape, splits):
    """Stride-2 1x1 wgrad (projection shortcut, reference networks/resnet_big.py:50-55) on the
    pipelined 1x1 kernel (cfg 10): output widths 16 / 8 / 4 (a 32-pixel step is 2 / 4 / 8
    output rows, crossing images at 4 and 8) and 7 / 14 / 28 / 12 (steps that are not whole
    rows: the GEN instantiation's per-step g / Q), vs fp32 torch; direct, split-K, auto, sink."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 1)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, stride=2)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    dw = m.conv_wgrad(dyh, xh, 1, 1, 2, 0, splits, 10)
    assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
    sink = torch.full((K, 1, 1, C), 0.25, device=gpu)
    m.conv_wgrad(dyh, xh, 1, 1, 2, 0, splits, 10, sink, True)
    assert _rel(sink - 0.25, dw.float()) < 1e-5
    if splits == 0:
        assert torch.equal(m.conv_wgrad(dyh, xh, 1, 1, 2, 0, 0, -1), dw)


def test_conv_large_m(gpu):
    """Layer-1 scale (M = 512·32·32) against torch bf16 conv."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    x, w = _mk(64, 32, 32, 64, 64, 3)
    ref = F.conv2d(x.float(), w.float(), padding=1)
    y, _ = m.conv_fwd(x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous(), 1, 1, False, -1)
    assert _rel(y.permute(0, 3, 1, 2), ref) < 1e-2


@pytest.mark.parametrize("shape", [(2, 9, 7, 64, 64, 3, 2, 1), (3, 7, 9, 64, 128, 1, 2, 0), (2, 10, 10, 64, 64, 3, 3, 1)])
def test_conv_dgrad_strided_odd(gpu, shape):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    xf = x.float().requires_grad_(True)
    out = F.conv2d(xf, w.float(), stride=st, padding=pad)
    dy = torch.randn_like(out).bfloat16()
    (dx_ref,) = torch.autograd.grad(out, xf, dy.float())
    dx = m.conv_dgrad(dy.permute(0, 2, 3, 1).contiguous(), w.permute(1, 2, 3, 0).contiguous(), H, W, st, pad, -1)
    assert _rel(dx.permute(0, 3, 1, 2), dx_ref) < 1e-2


def test_conv_wgrad_into_sink_accumulate(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = 4, 8, 8, 64, 128, 3, 1, 1
    x, w = _mk(N, H, W, C, K, R)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf, stride=st, padding=pad)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    sink = torch.ones(K, C, R, R, device=gpu).contiguous(memory_format=torch.channels_last)
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    m.conv_wgrad(dyh, xh, R, R, st, pad, 3, -1, sink, True)
    assert _rel(sink - 1, dw_ref) < 5e-3
    m.conv_wgrad(dyh, xh, R, R, st, pad, 1, -1, sink, False)
    assert _rel(sink, dw_ref) < 5e-3


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] % 8 == 0 and s[3] > 8])
@pytest.mark.parametrize("cfg", [0, 3])
def test_conv_bn_relu_prologue(gpu, shape, cfg):
    """conv_fwd / conv_wgrad with in_scale/in_shift == the same conv on the materialised
    relu(y·scale + shift) (bf16), incl. zero padding taps staying zero."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    y, w = _mk(N, H, W, C, K, R, seed=3)
    yh = y.permute(0, 2, 3, 1).contiguous()
    wh = w.permute(0, 2, 3, 1).contiguous()
    g = torch.Generator(device="cpu").manual_seed(4)
    sc = (torch.rand(C, generator=g) + 0.5).cuda()
    sh = (torch.randn(C, generator=g) * 0.5).cuda()
    a = torch.relu(yh.float() * sc + sh).bfloat16()
    ref, slab_ref = m.conv_fwd(a, wh, st, pad, True, cfg)
    out, slab = m.conv_fwd(yh, wh, st, pad, True, cfg, sc, sh)
    assert _rel(out, ref) < 1e-2
    s_ref, s = m.bn_stats_reduce(slab_ref), m.bn_stats_reduce(slab)
    assert torch.allclose(s, s_ref, rtol=1e-3, atol=1e-1)
    dy = torch.randn(out.shape, generator=g).cuda().bfloat16()
    dw_ref = m.conv_wgrad(dy, a, R, R, st, pad, 0, cfg)
    dw = m.conv_wgrad(dy, yh, R, R, st, pad, 0, cfg, None, False, sc, sh)
    assert _rel(dw, dw_ref) < 1e-2


def test_dgrad_masked_addend(gpu):
    """conv_dgrad(addend=g, addend_mask=bits) == conv_dgrad + g·[bit] (fused identity-shortcut
    gradient of a ReLU'd block output)."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    torch.manual_seed(9)
    N, H, W, C, K = 4, 8, 8, 64, 256
    dy = torch.randn(N, H, W, K, device=gpu).bfloat16()
    wt = (torch.randn(C, 1, 1, K, device=gpu) * 0.05).bfloat16()
    g = torch.randn(N, H, W, C, device=gpu).bfloat16()
    bits = torch.randint(0, 256, (g.numel() // 8,), dtype=torch.uint8, device=gpu)
    ref = m.conv_dgrad(dy, wt, H, W, 1, 0).float()
    keep = ((bits.long().unsqueeze(1) >> torch.arange(8, device=gpu)) & 1).reshape(g.shape).float()
    exp = ref + g.float() * keep
    out = m.conv_dgrad(dy, wt, H, W, 1, 0, -1, None, g, bits)
    assert _rel(out, exp) < 1e-2


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] & (s[3] - 1) == 0])   # bn backward: power-of-two C
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("mask", ["none", "bits", "affine"])
def test_dgrad_bn_stats_epilogue(gpu, shape, cfg, mask):
    """conv_dgrad_bnstat: dx identical to conv_dgrad; its slab sums to Σd·m, Σd·m·(y−μ)
    of the STORED dx (m: ReLU bitmask / y·msc+msh > 0 / none), and bn_bwd_coef_slab gives
    the coefficients of the unfused bn_bwd_reduce_coef."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, W, C, K, R, st, pad = shape
    x, w = _mk(N, H, W, C, K, R)
    P = (H + 2 * pad - R) // st + 1
    Q = (W + 2 * pad - R) // st + 1
    g = torch.Generator(device="cpu").manual_seed(3)
    dy = torch.randn(N, P, Q, K, generator=g).to(gpu).bfloat16()
    wt = w.permute(1, 2, 3, 0).contiguous()
    y = torch.randn(N, H, W, C, generator=g).to(gpu).bfloat16()
    mu = torch.randn(C, generator=g).to(gpu) * 0.1
    inv = torch.rand(C, generator=g).to(gpu) + 0.5
    gam = torch.randn(C, generator=g).to(gpu)
    msc = torch.randn(C, generator=g).to(gpu)
    msh = torch.randn(C, generator=g).to(gpu) * 0.1
    bits = torch.randint(0, 256, (y.numel() // 8,), dtype=torch.uint8, device=gpu)
    kw = {}
    if mask == "bits":
        kw = dict(mask_bits=bits)
    elif mask == "affine":
        kw = dict(msc=msc, msh=msh)
    dx, slab = m.conv_dgrad_bnstat(dy, wt, H, W, st, pad, cfg, ya=y, ma=mu, **kw)
    ref = m.conv_dgrad(dy, wt, H, W, st, pad, cfg)
    assert torch.equal(dx, ref)
    d = ref.double().reshape(-1, C)
    yy = y.double().reshape(-1, C)
    if mask == "bits":
        keep = ((bits.long().unsqueeze(1) >> torch.arange(8, device=gpu)) & 1).reshape(-1, C).double()
        d = d * keep
    elif mask == "affine":
        d = d * ((y.float() * msc + msh) > 0).reshape(-1, C).double()
    s = slab.double().sum(0)
    scale = d.abs().sum(0).clamp_min(1.0)
    assert ((s[0] - d.sum(0)).abs() / scale).max() < 1e-4
    assert ((s[1] - (d * (yy - mu.double())).sum(0)).abs() / (scale * 4)).max() < 1e-4
    # coefficients + dγ/dβ from the slab == the unfused reduction's
    kwr = {"bits": dict(outv=None), "affine": dict(outv=None, msc=msc, msh=msh), "none": dict(outv=None)}[mask]
    if mask == "bits":
        # the unfused kernel takes the bitmask as `outv` uint8 only through the executor; compare against
        # the masked tensor instead
        ref_in = (d.reshape(ref.shape)).bfloat16()
        ca = m.bn_bwd_reduce_coef(ref_in, None, y, mu, count=float(N * H * W), g_a=gam, inv_a=inv)
    else:
        ca = m.bn_bwd_reduce_coef(ref, ya=y, ma=mu, count=float(N * H * W), g_a=gam, inv_a=inv, **kwr)
    cs = m.bn_bwd_coef_slab(0, slab, float(N * H * W), gam, mu, inv)
    for a_, b_ in ((cs[0], ca[0]), (cs[2], ca[2]), (cs[3], ca[3])):
        assert torch.allclose(a_, b_, rtol=1e-3, atol=1e-3 * b_.abs().max().item() + 1e-5)


def test_dgrad_bn_stats_two_sets_with_addend(gpu):
    """Projection-shortcut form: two BN inputs (ya, yb) fed by the same dx, with the fused
    masked addend; 3-set slab."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    torch.manual_seed(5)
    N, H, W, C, K = 4, 8, 8, 64, 256
    dy = torch.randn(N, H, W, K, device=gpu).bfloat16()
    wt = (torch.randn(C, 1, 1, K, device=gpu) * 0.05).bfloat16()
    add = torch.randn(N, H, W, C, device=gpu).bfloat16()
    abits = torch.randint(0, 256, (add.numel() // 8,), dtype=torch.uint8, device=gpu)
    ya = torch.randn(N, H, W, C, device=gpu).bfloat16()
    yb = torch.randn(N, H, W, C, device=gpu).bfloat16()
    ma, mb = torch.randn(C, device=gpu) * 0.1, torch.randn(C, device=gpu) * 0.1
    bits = torch.randint(0, 256, (ya.numel() // 8,), dtype=torch.uint8, device=gpu)
    dx, slab = m.conv_dgrad_bnstat(dy, wt, H, W, 1, 0, -1, None, add, abits, ya, ma, yb, mb, bits)
    ref = m.conv_dgrad(dy, wt, H, W, 1, 0, -1, None, add, abits)
    assert torch.equal(dx, ref)
    keep = ((bits.long().unsqueeze(1) >> torch.arange(8, device=gpu)) & 1).reshape(-1, C).double()
    d = ref.double().reshape(-1, C) * keep
    s = slab.double().sum(0)
    sc = d.abs().sum(0).clamp_min(1.0)
    assert ((s[0] - d.sum(0)).abs() / sc).max() < 1e-4
    assert ((s[1] - (d * (ya.double().reshape(-1, C) - ma.double())).sum(0)).abs() / (4 * sc)).max() < 1e-4
    assert ((s[2] - (d * (yb.double().reshape(-1, C) - mb.double())).sum(0)).abs() / (4 * sc)).max() < 1e-4


@pytest.mark.parametrize("shape", [(4, 8, 8, 64, 128), (2, 9, 7, 32, 64)])
def test_dgrad_compact_subgrid_addend(gpu, shape):
    """conv_dgrad(addend=compact, addend_sub=2) == conv_dgrad(addend=the strided 1x1 shortcut's
    full dgrad): the shortcut gradient is added only at even (h, w), read from a compact
    [N, ceil(H/2), ceil(W/2), C] tensor; also through the BN-statistics variant."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    torch.manual_seed(11)
    N, H, W, C, K = shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy1 = torch.randn(N, H, W, K, device=gpu).bfloat16()          # c1 (1x1, stride 1) output grad
    wt1 = (torch.randn(C, 1, 1, K, device=gpu) * 0.05).bfloat16()
    dys = torch.randn(N, P, Q, 2 * K, device=gpu).bfloat16()      # shortcut (1x1, stride 2) output grad
    wts = (torch.randn(C, 1, 1, 2 * K, device=gpu) * 0.05).bfloat16()
    full = m.conv_dgrad(dys, wts, H, W, 2, 0)
    compact = m.conv_dgrad(dys, wts, P, Q, 1, 0)
    assert torch.equal(full[:, ::2, ::2, :], compact)
    ref = m.conv_dgrad(dy1, wt1, H, W, 1, 0, -1, None, full)
    out = m.conv_dgrad(dy1, wt1, H, W, 1, 0, -1, None, compact, None, 2)
    assert torch.equal(out, ref)
    y = torch.randn(N, H, W, C, device=gpu).bfloat16()
    mu = torch.zeros(C, device=gpu)
    r_ref = m.conv_dgrad_bnstat(dy1, wt1, H, W, 1, 0, -1, None, full, None, y, mu)
    r = m.conv_dgrad_bnstat(dy1, wt1, H, W, 1, 0, -1, None, compact, None, y, mu, addend_sub=2)
    assert torch.equal(r[0], r_ref[0]) and torch.allclose(r[1], r_ref[1], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(4, 16, 256, 64), (2, 8, 512, 128), (2, 8, 1024, 256), (3, 8, 256, 128)])
@pytest.mark.parametrize("cfg", [-1, 1, 4, 6])
def test_conv_dgrad_cat(gpu, shape, cfg):
    """K-concatenated stride-1 1x1 dgrad (BN3 fold: da2 = dz·Wd + a2·Mx + b in one GEMM,
    igemm.hip a2 operand) vs fp32 torch, on the DEPTH 3 (cfgs 1, 4) and DEPTH 6 (cfg 6)
    LDS-DMA loops; with the BN-statistics epilogue the same dx and the slab's sums."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, K, K2 = shape
    C = K2
    g = torch.Generator(device="cpu").manual_seed(3)
    dy = torch.randn(N, H, H, K, generator=g).bfloat16().to(gpu)
    a2 = torch.randn(N, H, H, K2, generator=g).bfloat16().to(gpu)
    wcat = (torch.randn(C, 1, 1, K + K2, generator=g) / (K + K2) ** 0.5).bfloat16().to(gpu)
    bias = torch.randn(C, generator=g).to(gpu)
    wf = wcat.float().reshape(C, K + K2)
    ref = dy.float().reshape(-1, K) @ wf[:, :K].t() + a2.float().reshape(-1, K2) @ wf[:, K:].t() + bias
    dx = m.conv_dgrad_cat(dy, wcat, a2, bias, cfg)[0]
    assert dx.shape == (N, H, H, C)
    assert _rel(dx.reshape(-1, C), ref) < 1e-2
    ya = torch.randn(N, H, H, C, generator=g).bfloat16().to(gpu)
    ma = torch.randn(C, generator=g).to(gpu)
    dx2, slab = m.conv_dgrad_cat(dy, wcat, a2, bias, cfg, ya, ma)
    assert torch.equal(dx2, dx)
    s = slab.double().sum(0)
    d = dx.double().reshape(-1, C)
    assert torch.allclose(s[0], d.sum(0), rtol=1e-4, atol=1e-2)
    assert torch.allclose(s[1], (d * (ya.double().reshape(-1, C) - ma.double())).sum(0), rtol=1e-4, atol=1e-1)


@pytest.mark.parametrize("shape", [(2, 8, 512, 256), (8, 4, 128, 512), (16, 16, 256, 256), (4, 8, 2048, 512),
                                   (3, 8, 256, 768)])
@pytest.mark.parametrize("splits", [1, 5, 0])
def test_wgrad1x1_big_matches_128row_kernel(gpu, shape, splits):
    """The 256-row LDS-DMA 1x1 wgrad (wgrad1x1_big_kernel: 4-slot DMA ring, three steps in
    flight) vs fp32 torch and vs the 128-row register-ring kernel on the same shapes (256- and
    128-wide column tiles, split counts whose last split is short, accumulation into a sink)."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 1)
    wf = w.float().requires_grad_(True)
    out = F.conv2d(x.float(), wf)
    dy = torch.randn_like(out).bfloat16()
    (dw_ref,) = torch.autograd.grad(out, wf, dy.float())
    dyh, xh = dy.permute(0, 2, 3, 1).contiguous(), x.permute(0, 2, 3, 1).contiguous()
    prev = m.wgrad1x1_big_set(2)   # every eligible shape (the default rule skips small GEMMs)
    try:
        dw = m.conv_wgrad(dyh, xh, 1, 1, 1, 0, splits, 10)
        assert _rel(dw.permute(0, 3, 1, 2), dw_ref) < 5e-3
        sink = torch.full((K, 1, 1, C), 0.25, device=gpu)
        m.conv_wgrad(dyh, xh, 1, 1, 1, 0, splits, 10, sink, True)
        assert _rel(sink - 0.25, dw.float()) < 1e-5
        m.wgrad1x1_big_set(0)
        dw_old = m.conv_wgrad(dyh, xh, 1, 1, 1, 0, splits, 10)
        assert _rel(dw, dw_old) < 1e-5
    finally:
        m.wgrad1x1_big_set(prev)


@pytest.mark.parametrize("mode,shape", [("fwd", (8, 8, 256, 1024)), ("fwd", (16, 16, 128, 512)),
                                        ("fwd", (4, 8, 200, 256)), ("dgrad", (8, 8, 1024, 256)),
                                        ("dgrad", (16, 16, 512, 128))])
def test_single_stage_loop_matches_two_stage(gpu, mode, shape):
    """The single-stage DEPTH 3 loop over several K-tiles (igemm_one_k_set: forward 1x1 GEMMs
    with K <= 256 by default) issues the same MFMAs in the same order as the two-stage loop,
    so outputs and BN statistics are bit-identical; also vs fp32 torch."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    N, H, C, K = shape
    x, w = _mk(N, H, H, C, K, 1)
    xh, wh = x.permute(0, 2, 3, 1).contiguous(), w.permute(0, 2, 3, 1).contiguous()
    mi = 0 if mode == "fwd" else 1
    outs = []
    for lim in (64, 4096):
        prev = m.igemm_one_k_set(mi, lim)
        try:
            if mode == "fwd":
                outs.append(m.conv_fwd(xh, wh, 1, 0, True, -1))
            else:
                dy = torch.randn(N, H, H, K, device=gpu, generator=torch.Generator(gpu).manual_seed(3)).bfloat16()
                outs.append([m.conv_dgrad(dy, wh.permute(3, 1, 2, 0).contiguous(), H, H, 1, 0, -1)])
        finally:
            m.igemm_one_k_set(mi, prev)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    if mode == "fwd":
        ref = F.conv2d(x.float(), w.float())
        assert _rel(outs[1][0].permute(0, 3, 1, 2), ref) < 1e-2


TRACE_SCRIPT = r"""
import json, torch
from simclr_pytorch_distributed_amd.ops import _ext
m = _ext.require()
x = torch.randn(1, 8, 8, 64, device="cuda").bfloat16()
w = (torch.randn(64, 1, 1, 64, device="cuda") * 0.1).bfloat16()
m.conv_fwd(x, w, 1, 0, True, 3)
fwd = m.igemm_trace()[0].tolist()
m.conv_dgrad(x, w.permute(3, 1, 2, 0).contiguous(), 8, 8, 1, 0, 3)
dgrad = m.igemm_trace()[0].tolist()
print("TRACE " + json.dumps([fwd, dgrad]))
"""


def test_igemm_trace_follows_the_last_traced_family(gpu):
    """The forward and data-gradient kernels live in different translation units, each with
    its own trace buffer; igemm_trace() must read the buffer of the unit that launched last
    (a copy from another unit's buffer would return zeros or a stale timeline). One 1x1
    conv at N=1, 8x8, 64 -> 64, cfg 3, forward then stride-1 dgrad, in a child process
    (SDX_IGEMM_TRACE is read once, at the first launch): wave 0's start stamp (slot 0) and
    end stamp (slot -2) are non-zero and ordered after each, and the dgrad's differ from
    the forward's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SDX_IGEMM_TRACE="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", TRACE_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    fwd, dgrad = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TRACE ")][-1][6:])
    for t in (fwd, dgrad):
        assert 0 < t[0] < t[-2], (t[0], t[-2])
    assert dgrad[0] != fwd[0] and dgrad[-2] != fwd[-2], (fwd[0], fwd[-2], dgrad[0], dgrad[-2])
