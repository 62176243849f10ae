"""fp64 oracle of one residual block (BasicBlock / Bottleneck), whole and stage by stage.

The math is the model definition the executor cites (networks/resnet_big.py:7-67):

    BasicBlock   out = relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x))
                 conv1 3x3 / stride / pad 1, conv2 3x3 / 1 / pad 1
    Bottleneck   out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + shortcut(x))
                 conv1 1x1, conv2 3x3 / stride / pad 1, conv3 1x1
    shortcut     identity, or bn_s(conv_s(x)) with conv_s 1x1 / stride

with torch BatchNorm2d semantics: training normalises with the batch mean and the biased batch
variance and moves the running buffers by ``momentum`` towards the mean and the UNBIASED
variance; eval normalises with the running buffers and changes nothing.

Everything is plain torch float64 on the CPU, activations NHWC ``[N, H, W, C]``, weights
``[K, R, S, C]`` (conv_oracle's layouts). Nothing of the package is imported. The single
operations are the ones tests/conv_oracle.py and tests/bn_oracle.py already state; this module
only strings them together, which is the thing under test.

Two forms:

* ``forward`` / ``backward``: the whole block in exact float64, no rounding anywhere.
  tests/test_block_oracle.py holds ``backward`` to torch autograd (float64) at 1e-12.
* the **stage functions** (``conv_stage``, ``bn_stage``, ``act_stage``, ``bn_bwd_stage``,
  ``dgrad_stage``, ``wgrad_stage``): one operation each, taking its inputs as given, so that a
  test can feed them the executor's own stored bf16 tensors (teacher forcing) and compare one
  rounding step at a time. ``forward`` / ``backward`` are compositions of exactly these.
"""
from __future__ import annotations

import torch

import bn_oracle as B
import conv_oracle as C

F64 = torch.float64


class Spec:
    """Geometry of a block. ``convs``: (K, R, C, stride, pad) per conv in the executor's order
    conv1, conv2, (conv3), (shortcut); ``bn_rows(i, N, H, W)``: the row count of BN i."""

    def __init__(self, bottleneck, proj, stride, cin, mid, cout):
        self.bottleneck, self.proj, self.stride = bottleneck, proj, stride
        self.cin, self.mid, self.cout = cin, mid, cout
        assert proj or (stride == 1 and cin == cout)
        if bottleneck:
            self.convs = [(mid, 1, cin, 1, 0), (mid, 3, mid, stride, 1), (cout, 1, mid, 1, 0)]
        else:
            assert mid == cout
            self.convs = [(cout, 3, cin, stride, 1), (cout, 3, cout, 1, 1)]
        if proj:
            self.convs.append((cout, 1, cin, stride, 0))
        self.nconv = 3 if bottleneck else 2
        self.nbn = len(self.convs)

    def out_hw(self, H, W):
        return C.out_size(H, 3, self.stride, 1), C.out_size(W, 3, self.stride, 1)

    def bn_rows(self, i, N, H, W):
        """Pixels BN i normalises over: a bottleneck's bn1 sees the input grid, every other BN
        (the shortcut's included) the output grid."""
        P, Q = self.out_hw(H, W)
        return N * H * W if (self.bottleneck and i == 0) else N * P * Q


def dgrad_layout(w):
    """[K, R, S, C] -> [C, R, S, K]"""
    return w.permute(3, 1, 2, 0).contiguous()


# ---------------------------------------------------------------- stage functions -------------

def conv_stage(x, w, stride, pad):
    """-> dict(s, mag, sums): the accumulators, Σ|x·w| per output element, and (Σs, Σs²) over the
    pixels (the statistics are taken from the accumulators)."""
    s = C.fwd_acc(x, w, stride, pad)
    mag = C.fwd_acc(x.to(F64).abs(), w.to(F64).abs(), stride, pad)
    return dict(s=s, mag=mag, sums=B.stats(s))


def bn_stage(sums, count, gamma, beta, eps, momentum, rm=None, rv=None):
    return B.finalize(sums, count, gamma, beta, eps, momentum, rm, rv)


def eval_stage(gamma, beta, rm, rv, eps):
    return B.eval_affine(gamma, beta, rm, rv, eps)


def act_stage(y, sc, sh, r=None, sc2=None, sh2=None, res_mode=0):
    """relu(y·sc + sh [+ r·sc2 + sh2 | + r]) -> (z, T)"""
    return B.apply(y, sc, sh, r, sc2, sh2, res_mode, relu=True)


def bn_bwd_stage(dout, mask_source, y, mu, iv, gamma, count, yb=None, mu_b=None, iv_b=None, gamma_b=None,
                 sums=None):
    """BN (+ a second BN fed by the same gradient) + ReLU backward of [N, H, W, C] tensors.
    ``sums``: use these [2|3, C] sums instead of the stage's own (a statistics slab handed in).
    -> dict(sums, abs_sums, dz, ca, cb, dya, Ta, dyb, Tb); ca / cb as bn_oracle.coef."""
    Cn = dout.shape[-1]
    f = lambda t: None if t is None else t.to(F64).reshape(-1, Cn)
    own, abs_sums, dz = B.bwd_sums(f(dout), mask_source, f(y), mu, f(yb), mu_b)
    s = own if sums is None else sums.to(F64)
    o = dict(sums=s, own_sums=own, abs_sums=abs_sums, dz=dz.reshape(dout.shape), cb=None, dyb=None, Tb=None)
    o["ca"] = B.coef(s, count, gamma, mu, iv, 1.0, 0)
    for key, yy, si, g, m, v in (("a", y, 0, gamma, mu, iv), ("b", yb, 1, gamma_b, mu_b, iv_b)):
        if yy is None:
            continue
        c = B.coef(s, count, g, m, v, 1.0, si)
        o["c" + key] = c
        o["dy" + key] = (c["A"] * dz + c["D"] * f(yy) + c["E"]).reshape(dout.shape)
        o["T" + key] = ((c["A"] * dz).abs() + (c["D"] * f(yy)).abs() + c["E"].abs()).reshape(dout.shape)
    return o


def dgrad_stage(dy, wt, H, W, stride, pad):
    """-> (acc, mag): the data gradient and Σ|dy·w| per element."""
    return (C.dgrad_acc(dy, wt, H, W, stride, pad),
            C.dgrad_acc(dy.to(F64).abs(), wt.to(F64).abs(), H, W, stride, pad))


def wgrad_stage(dy, x, R, stride, pad):
    """-> (dW, mag)"""
    return (C.wgrad(dy, x, R, R, stride, pad), C.wgrad(dy.to(F64).abs(), x.to(F64).abs(), R, R, stride, pad))


def subgrid(t, s, H, W):
    """A compact [N, P, Q, C] tensor placed at h, w = 0 mod s of an [N, H, W, C] grid."""
    full = torch.zeros(t.shape[0], H, W, t.shape[3], dtype=F64)
    full[:, ::s, ::s] = t.to(F64)
    return full


# ---------------------------------------------------------------- the whole block -------------

def forward(spec, x, ws, bns, training, eps, momentum):
    """ws: forward weights (spec.convs order); bns: [gamma, beta, running_mean, running_var] per
    BN. -> dict(y: [y1, y2, (y3), (ys)], a: [a1, (a2)], st: per-BN finalize dicts (training) or
    dict(scale, shift) (eval), out, pre)."""
    x = x.to(F64)
    N, H, W, _ = x.shape
    y, a, st = [None] * spec.nbn, [], [None] * spec.nbn

    def bn(i, acc):
        g, b, rm, rv = bns[4 * i:4 * i + 4]
        if training:
            return bn_stage(B.stats(acc), spec.bn_rows(i, N, H, W), g, b, eps, momentum, rm, rv)
        sc, sh = eval_stage(g, b, rm, rv, eps)
        return dict(scale=sc, shift=sh)

    cur = x
    for i in range(spec.nconv):
        K, R, Cc, s, p = spec.convs[i]
        y[i] = conv_stage(cur, ws[i], s, p)["s"]
        st[i] = bn(i, y[i])
        if i < spec.nconv - 1:
            cur = act_stage(y[i], st[i]["scale"], st[i]["shift"])[0]
            a.append(cur)
    L = spec.nconv - 1
    if spec.proj:
        n = spec.nconv
        y[n] = conv_stage(x, ws[n], spec.stride, 0)["s"]
        st[n] = bn(n, y[n])
        out, _ = act_stage(y[L], st[L]["scale"], st[L]["shift"], y[n], st[n]["scale"], st[n]["shift"], 1)
    else:
        out, _ = act_stage(y[L], st[L]["scale"], st[L]["shift"], x, None, None, 2)
    return dict(y=y, a=a, st=st, out=out)


def backward(spec, x, ws, bns, fwd, dout):
    """Training-mode backward of ``forward``'s result. -> dict(dx, dw [per conv], dgamma, dbeta
    [per BN], and the intermediates dz, dy3 / dys (as dy[i]), da2, da1 (as da[i]))."""
    x = x.to(F64)
    N, H, W, _ = x.shape
    P, Q = spec.out_hw(H, W)
    y, a, st = fwd["y"], fwd["a"], fwd["st"]
    L, n = spec.nconv - 1, spec.nconv
    dw, dg, db, dy, da = [None] * spec.nbn, [None] * spec.nbn, [None] * spec.nbn, [None] * spec.nbn, [None] * n
    g = lambda i: bns[4 * i]
    rows = lambda i: spec.bn_rows(i, N, H, W)
    if spec.proj:
        r = bn_bwd_stage(dout, ("act", fwd["out"]), y[L], st[L]["mean"], st[L]["invstd"], g(L), rows(L),
                         y[n], st[n]["mean"], st[n]["invstd"], g(n))
        dy[n], dg[n], db[n] = r["dyb"], r["cb"]["dgamma"], r["cb"]["dbeta"]
    else:
        r = bn_bwd_stage(dout, ("act", fwd["out"]), y[L], st[L]["mean"], st[L]["invstd"], g(L), rows(L))
    dz = r["dz"]
    dy[L], dg[L], db[L] = r["dya"], r["ca"]["dgamma"], r["ca"]["dbeta"]
    ins = [x] + a                                # conv i reads ins[i]
    for i in range(L, 0, -1):
        K, R, Cc, s, p = spec.convs[i]
        dw[i] = wgrad_stage(dy[i], ins[i], R, s, p)[0]
        da[i] = dgrad_stage(dy[i], dgrad_layout(ws[i].to(F64)), ins[i].shape[1], ins[i].shape[2], s, p)[0]
        j = i - 1
        r = bn_bwd_stage(da[i], ("affine", st[j]["scale"], st[j]["shift"]), y[j], st[j]["mean"], st[j]["invstd"],
                         g(j), rows(j))
        dy[j], dg[j], db[j] = r["dya"], r["ca"]["dgamma"], r["ca"]["dbeta"]
    K, R, Cc, s, p = spec.convs[0]
    dw[0] = wgrad_stage(dy[0], x, R, s, p)[0]
    dx = dgrad_stage(dy[0], dgrad_layout(ws[0].to(F64)), H, W, s, p)[0]
    if spec.proj:
        dw[n] = wgrad_stage(dy[n], x, 1, spec.stride, 0)[0]
        dx = dx + dgrad_stage(dy[n], dgrad_layout(ws[n].to(F64)), H, W, spec.stride, 0)[0]
    else:
        dx = dx + dz
    return dict(dx=dx, dw=dw, dgamma=dg, dbeta=db, dz=dz, dy=dy, da=da)
