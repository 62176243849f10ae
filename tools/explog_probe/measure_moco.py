#!/usr/bin/env python3
"""Error of the device __expf on the fp32 arguments the MoCo backward gives it, against fp64.

moco.hip's backward forms p = __expf(s·fp32(1/T) − lse), an argument down to −2/T − log(K + 1): below the
|x| <= 30.3 that measure.py covered for the SwAV kernels. For every shape and temperature of
tests/test_gpu_moco.py the kernels' own q̂ and lse are taken (moco_fwd), s is the fp32 of the fp64 product
q̂·Qᵀ (the kernel's own s differs from it by its GEMM error, which moves an argument by < 1e-5), and the
argument is formed in fp32 with one rounding as the kernel's fma does. Printed per case and overall: the
worst |δ| of __expf(x) = exp(x)(1 + δ) in units of (1 + |x|)·u, over all arguments and over |x| > 30.3
alone. Needs a GPU.

    python tools/explog_probe/measure_moco.py PROBE_BINARY
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

import test_gpu_moco as T  # noqa: E402
from measure import U, probe  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext  # noqa: E402


def main():
    binary = os.path.abspath(sys.argv[1])
    m = _ext.require()
    dev = torch.device("cuda:0")
    worst = [0.0, 0.0]
    for N, D, K in T.SHAPES:
        for temp in T.TEMPS:
            q, k, queue = (t.to(dev) for t in T.inputs(N, D, K))
            _, lse, _, qhat, _, _ = m.moco_fwd(q, k, queue, temp, 0)
            Q = queue[0].cpu().double() + queue[1].cpu().double()
            s = (qhat.cpu().double() @ Q.t()).float().double()
            x = (s * T.f32_value(1 / temp) - lse.cpu().double()[:, None]).float()
            y = probe(binary, "exp", x).double()
            d = (y / x.double().exp() - 1).abs() / ((1 + x.double().abs()) * U)
            far = x.abs() > T.PROBED
            a, b = d.max().item(), d[far].max().item() if far.any() else 0.0
            print(f"N={N:4d} D={D:4d} K={K:5d} T={temp:4.2f}  x in [{x.min().item():7.2f}, {x.max().item():6.2f}]  "
                  f"|δ| <= {a:.4f}·(1 + |x|)·u   beyond {T.PROBED}: {int(far.sum())} arguments, {b:.4f}·(1 + |x|)·u",
                  flush=True)
            worst = [max(worst[0], a), max(worst[1], b)]
    print(f"worst: __expf |δ| <= {worst[0]:.4f}·(1 + |x|)·u, beyond {T.PROBED}: {worst[1]:.4f}·(1 + |x|)·u")


if __name__ == "__main__":
    main()
