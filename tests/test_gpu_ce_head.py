"""The trainable classifier + cross-entropy node (csrc/kernels/linear_ce.hip ce_head_bwd,
ops/ce_head.py) against an fp64 torch oracle: F.linear + F.cross_entropy(reduction="mean") with
autograd on x, W and b.

Shapes: B in {1, 5, 37} x K in {64, 512, 2048} x C in {1, 3, 10, 70, 1000} — a partial 4-row
block, KJ = 1 and 32, idle waves (C < 4), the wave-strided class loop with C % 4 != 0, the
lane-strided softmax loop (C > 64), near kMaxClasses.

Tolerance, per quantity: fp32 torch's own error against the oracle on the same inputs is
measured; the kernel is allowed 4 x that (its summation order differs) plus one fp32 ulp of the
result's magnitude (2^-23 x max |oracle|). Both errors are printed.

Worst kernel error / allowance seen on an MI355X over the 45 shapes: 0.609 (dX at B = 1,
K = 2048, C = 1000), then 0.573 and 0.539 (dX at C = 1000), 0.468 (db at B = 37, K = 512, C = 10);
the loss's worst is 0.325. With the row statistics summed in fp32 the mean loss at B = 37,
K = 2048, C = 10 stood at 1.12 (5.1e-7 against fp32 torch's 3.2e-8); the backward launch now
sums them in fp64.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(B, K, C) for K in (64, 512, 2048) for C in (1, 3, 10, 70, 1000) for B in (1, 5, 37)]
ULP = 2.0 ** -23


def _inputs(B, K, C, dev, seed=0):
    g = torch.Generator().manual_seed(1000 * K + 10 * C + B + seed)
    x = torch.randn(B, K, generator=g).relu()
    W = torch.randn(C, K, generator=g) / K ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    return x.to(dev), W.to(dev), b.to(dev), y.to(dev)


def _torch_ce(x, W, b, y, dtype):
    x, W, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, W, b))
    z = F.linear(x, W, b)
    loss = F.cross_entropy(z, y, reduction="mean")
    dx, dW, db = torch.autograd.grad(loss, [x, W, b])
    return {"loss": loss.detach(), "logits": z.detach(), "dX": dx, "dW": dW, "db": db}


def _hits(z, y):
    above = (z > z.gather(1, y[:, None])).sum(1)
    return float((above < 1).sum()), float((above < 5).sum())


def _native(x, W, b, y, gout=None):
    """One forward + backward of the node with fresh zeroed sinks; every output as a tensor."""
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce_logits
    fc = torch.nn.Linear(W.shape[1], W.shape[0]).to(x.device)
    with torch.no_grad():
        fc.weight.copy_(W)
        fc.bias.copy_(b)
    xr = x.detach().clone().requires_grad_(True)
    loss, stats, logits = classifier_ce_logits(xr, fc, y)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_ClassifierCE")
    loss.backward(gout)
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "logits": logits, "dX": xr.grad, "dW": fc.weight.grad, "db": fc.bias.grad,
            "stats": stats}


@pytest.mark.parametrize("B,K,C", SHAPES)
def test_ce_head_matches_fp64_oracle(gpu, B, K, C):
    x, W, b, y = _inputs(B, K, C, gpu)
    ref = _torch_ce(x, W, b, y, torch.float64)
    t32 = _torch_ce(x, W, b, y, torch.float32)
    got = _native(x, W, b, y)
    worst = 0.0
    fails = []
    for q in ("loss", "logits", "dX", "dW", "db"):
        e32 = float((t32[q].double() - ref[q]).abs().max())
        ek = float((got[q].double() - ref[q]).abs().max())
        allow = 4.0 * e32 + ULP * float(ref[q].abs().max())
        ratio = ek / allow if allow > 0 else (0.0 if ek == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"B={B} K={K} C={C} {q}: kernel err {ek:.3e}, fp32 torch err {e32:.3e}, allowed {allow:.3e}, "
              f"ratio {ratio:.3f}")
        if ek > allow:
            fails.append(q)
    print(f"B={B} K={K} C={C} worst ratio {worst:.3f}")
    h1, h5 = _hits(ref["logits"], y)
    assert (float(got["stats"][1]), float(got["stats"][2])) == (h1, h5)
    assert abs(float(got["stats"][0]) / B - float(got["loss"])) <= ULP * abs(float(got["loss"]))
    assert not fails, fails


def test_ce_head_accumulates_into_views(gpu):
    """dW / db are views inside a larger buffer: sentinels around them stay, a second backward
    without zeroing doubles every element bit for bit."""
    m = __import__("simclr_pytorch_distributed_amd.ops._ext", fromlist=["require"]).require()
    B, K, C = 37, 512, 70
    x, W, b, y = _inputs(B, K, C, gpu)
    buf = torch.full((8 + C * K + 8 + C + 8,), 123.25, device=gpu)
    dW = buf[8:8 + C * K].view(C, K)
    db = buf[8 + C * K + 8:8 + C * K + 8 + C]
    dW.zero_()
    db.zero_()
    one = torch.ones((), device=gpu)
    logits, dz, rowstat, stats, loss = m.ce_head_fwd(x, W, b, y, False)
    dx1 = m.ce_head_bwd(x, dz, W, one, rowstat, stats, loss, dW, db, True)
    torch.cuda.synchronize()
    first = buf.clone()
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[8:8 + C * K] = False
    outside[8 + C * K + 8:8 + C * K + 8 + C] = False
    assert int(outside.sum()) == 24 and bool((buf[outside] == 123.25).all())
    assert float(dW.abs().max()) > 0 and float(db.abs().max()) > 0
    dx2 = m.ce_head_bwd(x, dz, W, one, rowstat, stats, loss, dW, db, True)
    torch.cuda.synchronize()
    assert bool((buf[outside] == 123.25).all())
    assert torch.equal(buf[~outside], 2.0 * first[~outside]) and torch.equal(dx1, dx2)
    ref = _torch_ce(x, W, b, y, torch.float64)
    assert torch.allclose(dW.double(), 2.0 * ref["dW"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("B,K,C", [(37, 512, 70), (5, 2048, 1000)])
def test_ce_head_upstream_gradient_and_determinism(gpu, B, K, C):
    x, W, b, y = _inputs(B, K, C, gpu)
    a = _native(x, W, b, y)
    a2 = _native(x, W, b, y)
    for q in ("loss", "logits", "dX", "dW", "db", "stats"):
        assert torch.equal(a[q], a2[q]), q                       # bit-identical from run to run
    h = _native(x, W, b, y, torch.full((), 0.5, device=gpu))
    for q in ("dX", "dW", "db"):
        assert torch.equal(h[q], 0.5 * a[q]), q                  # bitwise half
    assert torch.equal(h["loss"], a["loss"])


def test_ce_head_no_grad_forward_and_frozen_classifier(gpu):
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
    B, K, C = 5, 64, 10
    x, W, b, y = _inputs(B, K, C, gpu)
    fc = torch.nn.Linear(K, C).to(gpu)
    with torch.no_grad():
        fc.weight.copy_(W)
        fc.bias.copy_(b)
        loss, stats = classifier_ce(x, fc, y)                    # reduced by the forward itself
    ref = _torch_ce(x, W, b, y, torch.float64)
    assert loss.grad_fn is None and abs(float(loss) - float(ref["loss"])) < 1e-5
    assert abs(float(stats[0]) - B * float(ref["loss"])) < 1e-4
    for p in fc.parameters():
        p.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    loss, _ = classifier_ce(xr, fc, y)
    loss.backward()
    assert fc.weight.grad is None and fc.bias.grad is None
    assert torch.allclose(xr.grad.double(), ref["dX"], rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("K,C", [(96, 10), (192, 10), (4096, 10), (32, 10), (64, 1025)])
def test_ce_head_rejects_unsupported_shapes(gpu, K, C):
    """K must be 64·2^j <= 2048 and C <= 1024: the ops raise before any launch (every output
    allocation they would have written stays untouched: nothing is returned), and the Python
    node takes the torch ops instead."""
    from simclr_pytorch_distributed_amd.ops import _ext
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce, supported
    m = _ext.require()
    B = 4
    x = torch.randn(B, K, device=gpu)
    W = torch.randn(C, K, device=gpu)
    b = torch.zeros(C, device=gpu)
    y = torch.zeros(B, dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError):
        m.ce_head_fwd(x, W, b, y, True)
    dW, db = torch.full_like(W, 7.0), torch.full_like(b, 7.0)
    with pytest.raises(RuntimeError):
        m.ce_head_bwd(x, torch.zeros(B, C, device=gpu), W, torch.ones((), device=gpu), torch.zeros(B, 3, device=gpu),
                      torch.zeros(3, device=gpu), torch.zeros((), device=gpu), dW, db, True)
    torch.cuda.synchronize()
    assert bool((dW == 7.0).all()) and bool((db == 7.0).all())
    fc = torch.nn.Linear(K, C).to(gpu)
    assert not supported(fc)
    xr = x.clone().requires_grad_(True)
    loss, _ = classifier_ce(xr, fc, y)
    assert torch.equal(loss, F.cross_entropy(F.linear(xr, fc.weight, fc.bias), y))
    # a misaligned or non-contiguous destination is refused as well
    K, C = 64, 10
    x, W, b, y = _inputs(B, K, C, gpu)
    out = m.ce_head_fwd(x, W, b, y, False)
    big = torch.zeros(C * K + 1, device=gpu)
    with pytest.raises(RuntimeError):
        m.ce_head_bwd(x, out[1], W, torch.ones((), device=gpu), out[2], out[3], out[4], big[1:].view(C, K),
                      torch.zeros(C, device=gpu), True)
    with pytest.raises(RuntimeError):
        m.ce_head_bwd(x, out[1], W, torch.ones((), device=gpu), out[2], out[3], out[4],
                      torch.zeros(K, C, device=gpu).t(), torch.zeros(C, device=gpu), True)
