"""GPU: the fused optimizer kernels (csrc/kernels/optim.hip) called directly on hand-made flat
fp32 buffers, against fp64 oracles: ``torch.optim.SGD`` on CPU double for ``sgd_step``, and for
``lars_step`` the definition in the kernel header written out in fp64 here:

    d = s*g + wd*p on adapted segments, d = s*g on the others
    trust = eta*||p||/||d|| if the segment is adapted and both norms are > 0, else 1
    buf = m*buf + lr*trust*d ;  p -= buf

Values have a wide dynamic range (randn * exp(2*randn)) so summation order and cancellation
matter. Every step is teacher-forced (the oracle restarts from the GPU's fp32 state) and is
held to a rounding bound derived from the oracle's own magnitudes, u = 2^-24; no fitted atol.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BLK = 4096


def _wide(gen, n):
    return (torch.randn(n, generator=gen, dtype=torch.float64)
            * torch.exp(2 * torch.randn(n, generator=gen, dtype=torch.float64))).float()


def _host(t):
    return t.detach().to("cpu", copy=True)


def _ext():
    from simclr_pytorch_distributed_amd.ops import _ext
    return _ext.require()


# ------------------------------------------------------------------------------- SGD ---------

def _sgd_oracle(p32, g32, buf32, lr, m, wd, s, nesterov):
    """One torch.optim.SGD step in float64 from the given fp32 state. Returns p', buf' and the
    magnitudes the bound needs."""
    p = torch.nn.Parameter(p32.double())
    p.grad = s * g32.double()
    opt = torch.optim.SGD([p], lr=lr, momentum=m, dampening=0, weight_decay=wd, nesterov=nesterov)
    if m > 0:
        opt.state[p]["momentum_buffer"] = buf32.double().clone()
    opt.step()
    sg, wp = (s * g32.double()).abs(), (wd * p32.double()).abs()
    d = s * g32.double() + wd * p32.double()
    b = opt.state[p]["momentum_buffer"] if m > 0 else d      # the kernel stores buf' = m*buf + d
    return p.detach(), b, d.abs(), sg + wp


def _check_sgd_step(got_p, got_b, p32, g32, buf32, lr, m, wd, s, nesterov, tag):
    p, b, dabs, dmag = _sgd_oracle(p32, g32, buf32, lr, m, wd, s, nesterov)
    # at most 6 roundings per element (wd*p, d, buf', the nesterov step, lr*step, p')
    bound_p = 8 * U * (p32.double().abs() + lr * ((1 + m) * b.abs() + dabs))
    # buf' = m*buf + d: the rounding of d (relative to |s*g| + |wd*p|, it may cancel), of m and of buf'
    bound_b = 8 * U * (b.abs() + dmag)
    ep, eb = (got_p.double() - p).abs(), (got_b.double() - b).abs()
    print(f"{tag}: worst err/bound p {float((ep / bound_p.clamp_min(1e-300)).max()):.3f} "
          f"buf {float((eb / bound_b.clamp_min(1e-300)).max()):.3f}")
    assert bool((ep <= bound_p).all()), (tag, int((ep > bound_p).sum()))
    assert bool((eb <= bound_b).all()), (tag, int((eb > bound_b).sum()))


N_TAIL = 4 * (3 * 256 * 2 + 37)          # 7 blocks of 256 float4, the last one ragged
N_CAP = 4 * (4096 * 256 + 5)             # one float4 block past the 4096-block grid cap

SGD_CASES = [  # n, nesterov, wd, gscale, momentum, max_blocks
    (4, False, 0.0, 1.0, 0.0, 0),
    (4 * 255, True, 1e-3, 0.125, 0.9, 0),
    (4 * 257, False, 1e-3, 1.0, 0.9, 1),
    (4 * 257, True, 1e-3, 0.125, 0.9, 3),
    (N_TAIL, True, 0.0, 1.0, 0.9, 3),
    (N_TAIL, False, 1e-3, 0.125, 0.0, 1),
    (N_TAIL, False, 0.0, 0.125, 0.9, 0),
    (N_CAP, True, 1e-3, 0.125, 0.9, 0),
]


@pytest.mark.parametrize("n,nesterov,wd,gscale,momentum,max_blocks", SGD_CASES)
def test_sgd_step_matches_torch_sgd_fp64(gpu, n, nesterov, wd, gscale, momentum, max_blocks):
    m = _ext()
    gen = torch.Generator().manual_seed(n % 1000 + 7 * max_blocks)
    p, buf = _wide(gen, n).to(gpu), _wide(gen, n).to(gpu)
    lr_t = torch.zeros(1, dtype=torch.float32, device=gpu)
    for step, lr in enumerate((0.1, 0.03, 0.5)):
        lr_t.fill_(lr)                                     # the device-resident lr changes between steps
        g = _wide(gen, n)
        p0, b0 = _host(p), _host(buf)
        m.sgd_step(p, g.to(gpu), buf, lr_t, momentum, wd, gscale, nesterov, max_blocks)
        _check_sgd_step(_host(p), _host(buf), p0, g, b0, float(lr_t.item()), momentum, wd, gscale, nesterov,
                        f"n={n} step {step}")


def test_sgd_step_on_a_slice_leaves_the_rest_untouched(gpu):
    """The call FusedSGD.apply_range makes: p[start:end], start a multiple of 4 but not of 4096."""
    m = _ext()
    gen = torch.Generator().manual_seed(5)
    n, start = 3 * BLK, 4 * 37
    end = start + N_TAIL
    p, g, buf = (_wide(gen, n).to(gpu) for _ in range(3))
    p0, b0 = _host(p), _host(buf)
    lr_t = torch.full((1,), 0.05, dtype=torch.float32, device=gpu)
    m.sgd_step(p[start:end], g[start:end], buf[start:end], lr_t, 0.9, 1e-3, 0.125, True, 3)
    p1, b1 = _host(p), _host(buf)
    for a, b in ((p0, p1), (b0, b1)):
        assert torch.equal(a[:start].view(torch.int32), b[:start].view(torch.int32))
        assert torch.equal(a[end:].view(torch.int32), b[end:].view(torch.int32))
    _check_sgd_step(p1[start:end], b1[start:end], p0[start:end], _host(g)[start:end], b0[start:end],
                    float(lr_t.item()), 0.9, 1e-3, 0.125, True, "slice")


def test_sgd_step_rejects_a_size_that_is_no_multiple_of_4(gpu):
    m = _ext()
    t = torch.zeros(6, dtype=torch.float32, device=gpu)
    lr_t = torch.full((1,), 0.1, dtype=torch.float32, device=gpu)
    with pytest.raises(RuntimeError):
        m.sgd_step(t, t.clone(), t.clone(), lr_t, 0.9, 0.0, 1.0, False, 0)


# ------------------------------------------------------------------------------- LARS --------

SEGS = [  # size, adapt, fill
    (1, 0, ""),
    (4096, 1, ""),
    (4097, 1, ""),
    (3 * 4096 + 17, 1, ""),
    (64, 0, ""),
    (5000, 1, "p0"),          # p == 0: pn = 0 on the first step
    (4096, 1, "g0"),          # g == 0: with wd = 0, dn = 0 on every step
    (1048576, 1, ""),         # 256 blocks
]
ETA = 1e-3


def _lars_table():
    offs, off = [], 0
    for size, _, _ in SEGS:
        offs.append(off)
        off += (size + BLK - 1) // BLK * BLK
    return offs, off


def _lars_state(seed):
    """CPU fp32 p, buf and three gradients; zero in the padding."""
    gen = torch.Generator().manual_seed(seed)
    offs, total = _lars_table()
    p, buf = torch.zeros(total), torch.zeros(total)
    grads = [torch.zeros(total) for _ in range(3)]
    for (size, _, fill), o in zip(SEGS, offs):
        if fill != "p0":
            p[o:o + size] = _wide(gen, size)
        buf[o:o + size] = _wide(gen, size)
        if fill != "g0":
            for g in grads:
                g[o:o + size] = _wide(gen, size)
    pad = torch.ones(total, dtype=torch.bool)
    for (size, _, _), o in zip(SEGS, offs):
        pad[o:o + size] = False
    return p, buf, grads, pad


def _norm_chain(nblk):
    """k: the longest chain of roundings a squared term passes through on its way into a
    segment's norm, read off seg_norms_kernel / lars_kernel: 16 terms per thread in sequence
    (the fma that squares the first one included), a 6-level wave butterfly and 3 additions over
    the 4 waves inside a block; then over the segment's nblk block partials ceil(nblk/256) - 1
    additions per thread, 6 butterfly levels and 3 additions over the waves."""
    return 16 + 6 + 3 + (math.ceil(nblk / 256) - 1) + 6 + 3


def _lars_oracle(p32, g32, buf32, lr, m, wd, s):
    """fp64 LARS step; returns p', buf', norms [nseg, 2] and the per-element / per-norm bounds."""
    offs, total = _lars_table()
    p, g, buf = p32.double(), g32.double(), buf32.double()
    p1, b1 = p.clone(), buf.clone()
    bound_p, bound_b = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    norms, norm_tol = [], []
    for (size, adapt, _), o in zip(SEGS, offs):
        sl = slice(o, o + size)
        w = wd if adapt else 0.0
        d = s * g[sl] + w * p[sl]
        # the kernel's fp32 d: rounding of wd (as a float), of wd*p, of s, and of the fma
        delta = 3 * U * ((s * g[sl]).abs() + (w * p[sl]).abs())
        n_p, n_d = float((p[sl] ** 2).sum()), float((d ** 2).sum())
        k = _norm_chain((size + BLK - 1) // BLK)
        tol_p = k * U * n_p
        tol_d = k * U * n_d + float((2 * d.abs() * delta + delta ** 2).sum()) * (1 + k * U)
        norms.append((n_p, n_d))
        norm_tol.append((tol_p, tol_d))
        trust, e_t = 1.0, 0.0
        if adapt and n_p > 0 and n_d > 0:
            trust = ETA * math.sqrt(n_p) / math.sqrt(n_d)
            # the square roots halve the norms' relative errors; sqrt, sqrt, eta as a float,
            # eta*pn and the division round once each, one more u for second-order terms
            e_t = 0.5 * (tol_p / n_p + tol_d / n_d) + 6 * U
        b1[sl] = m * buf[sl] + lr * trust * d
        p1[sl] = p[sl] - b1[sl]
        # lr*trust rounds once (with the trust error e_t), its product with d once, the final
        # fma once; m as a float and m*buf once each. (1 + 4u): the roundings act on the computed
        # values, not on the exact ones (second-order terms)
        bound_b[sl] = (1 + 4 * U) * (U * (b1[sl].abs() + 2 * (m * buf[sl]).abs())
                                     + lr * trust * ((e_t + 3 * U) * d.abs() + delta))
        bound_p[sl] = (1 + 4 * U) * (bound_b[sl] + U * p1[sl].abs())
    return p1, b1, norms, norm_tol, bound_p, bound_b


def _lars_call(m, gpu, p, g, buf, lr_t, momentum, wd, gscale, norms=None, partials=None):
    offs, total = _lars_table()
    seg_off = torch.tensor(offs, dtype=torch.int64, device=gpu)
    adapt = torch.tensor([a for _, a, _ in SEGS], dtype=torch.int32, device=gpu)
    # the outputs start as NaN: whatever the kernels do not write would show
    norms = torch.full((2 * len(SEGS),), float("nan"), device=gpu) if norms is None else norms
    partials = torch.full((2 * (total // BLK),), float("nan"), device=gpu) if partials is None else partials
    m.lars_step(p, g, buf, seg_off, adapt, lr_t, momentum, wd, gscale, ETA, norms, partials)
    return norms


@pytest.mark.parametrize("wd", [1e-3, 0.0])
def test_lars_step_matches_fp64_definition(gpu, wd):
    m = _ext()
    momentum, gscale = 0.9, 0.125
    p0, b0, grads, pad = _lars_state(3)
    p, buf = p0.to(gpu), b0.to(gpu)
    lr_t = torch.zeros(1, dtype=torch.float32, device=gpu)
    for step, (lr, g) in enumerate(zip((1.0, 0.3, 2.5), grads)):
        lr_t.fill_(lr)
        pc, bc = _host(p), _host(buf)
        norms = _lars_call(m, gpu, p, g.to(gpu), buf, lr_t, momentum, wd, gscale).cpu().double().view(-1, 2).clone()
        want_p, want_b, want_n, tol_n, bound_p, bound_b = _lars_oracle(pc, g, bc, float(lr_t.item()), momentum, wd,
                                                                       gscale)
        got_p, got_b = _host(p), _host(buf)
        # padding stays exactly zero
        assert not got_p[pad].any() and not got_b[pad].any()
        # norms within gamma_k = k * 2^-24 relative, k = _norm_chain(blocks of the segment): 34 for
        # every segment here (<= 256 blocks); the sum of d^2 also carries the rounding of d itself
        for i, ((n_p, n_d), (t_p, t_d)) in enumerate(zip(want_n, tol_n)):
            print(f"wd={wd} step {step} seg {i}: norm err/tol p {abs(norms[i, 0] - n_p) / max(t_p, 1e-300):.3f} "
                  f"d {abs(norms[i, 1] - n_d) / max(t_d, 1e-300):.3f}")
            assert abs(float(norms[i, 0]) - n_p) <= t_p, (step, i, float(norms[i, 0]), n_p)
            assert abs(float(norms[i, 1]) - n_d) <= t_d, (step, i, float(norms[i, 1]), n_d)
        if step == 0:
            assert want_n[5][0] == 0.0 and float(norms[5, 0]) == 0.0            # pn == 0
        if wd == 0.0:
            assert want_n[6][1] == 0.0 and float(norms[6, 1]) == 0.0            # dn == 0
        ep, eb = (got_p.double() - want_p).abs(), (got_b.double() - want_b).abs()
        print(f"wd={wd} step {step}: worst err/bound p {float((ep / bound_p.clamp_min(1e-300)).max()):.3f} "
              f"buf {float((eb / bound_b.clamp_min(1e-300)).max()):.3f}")
        assert bool((ep <= bound_p).all()), (step, int((ep > bound_p).sum()))
        assert bool((eb <= bound_b).all()), (step, int((eb > bound_b).sum()))


def test_lars_step_is_bit_reproducible(gpu):
    """Five runs from identical state, and one on a non-default stream: p, buf and norms are
    bit-identical (the 256-block segment included), two steps deep so a differing norm would
    also have to show in the parameters."""
    m = _ext()
    p0, b0, grads, _ = _lars_state(4)
    p0, b0, grads = p0.to(gpu), b0.to(gpu), [g.to(gpu) for g in grads]
    lr_t = torch.full((1,), 0.7, dtype=torch.float32, device=gpu)

    def run():
        p, buf = p0.clone(), b0.clone()
        out = []
        for g in grads[:2]:
            out.append(_lars_call(m, gpu, p, g, buf, lr_t, 0.9, 1e-3, 0.125).clone())
        return [p, buf] + out

    runs = [run() for _ in range(5)]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        runs.append(run())
    side.synchronize()
    torch.cuda.synchronize()
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_lars_step_rejects_a_size_that_is_no_multiple_of_4096(gpu):
    m = _ext()
    n = 4096 + 4
    t = torch.zeros(n, dtype=torch.float32, device=gpu)
    lr_t = torch.full((1,), 0.1, dtype=torch.float32, device=gpu)
    seg_off = torch.zeros(1, dtype=torch.int64, device=gpu)
    adapt = torch.ones(1, dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError):
        m.lars_step(t, t.clone(), t.clone(), seg_off, adapt, lr_t, 0.9, 0.0, 1.0, ETA,
                    torch.zeros(2, device=gpu), torch.zeros(2, device=gpu))
