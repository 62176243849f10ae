#!/usr/bin/env python3
"""Error of the device __expf / __logf on the fp32 arguments the SwAV kernels give them, against fp64.

For every shape and input of tests/test_gpu_swav.py the kernels' own S is taken (swav_prep,
swav_scores) and the arguments are formed in fp32 exactly as swav.hip forms them: (S − 1)·fp32(1/ε) for
the codes, (S − max)·fp32(1/τ) for the softmax, and Z = fp32(Σ exp) for the logarithm. The stand-alone
probe (explog_probe.hip, built with swav.hip's flags) evaluates the intrinsic once per element. Printed
per shape and overall: the worst |δ| of __expf(x) = exp(x)(1 + δ) in units of u = 2^-24 and of
(1 + |x|)·u, and the worst |ε| of __logf(l) = log l + ε in units of (1 + |log l|)·u. The test's K_EXP and
K_LOG are twice the overall worst of the (1 + |·|)·u figures. Needs a GPU.

    python tools/explog_probe/measure.py PROBE_BINARY
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_swav as T  # noqa: E402
from simclr_pytorch_distributed_amd.ops import _ext  # noqa: E402

U = 2.0 ** -24


def probe(binary, mode, x):
    with tempfile.TemporaryDirectory() as d:
        fi, fo = os.path.join(d, "in"), os.path.join(d, "out")
        x.numpy().astype(np.float32).tofile(fi)
        subprocess.run([binary, mode, fi, fo], check=True, timeout=120)
        return torch.from_numpy(np.fromfile(fo, dtype=np.float32)).reshape(x.shape)


def main():
    binary = os.path.abspath(sys.argv[1])
    m = _ext.require()
    dev = torch.device("cuda:0")
    worst = [0.0, 0.0, 0.0]
    for N, D, K in T.SHAPES:
        z1, z2, C = (t.to(dev) for t in T.inputs(N, D, K))
        zhat, _ = m.swav_prep(z1, z2, C)
        S = m.swav_scores(zhat, C, T.EPS)[0].cpu()[:, :K].contiguous()
        ie, it = torch.tensor(T.IE, dtype=torch.float32), torch.tensor(T.IT, dtype=torch.float32)
        xe = (S - 1.0) * ie
        xp = (S - S.max(1, keepdim=True).values) * it
        row = []
        for x in (xe, xp):
            y = probe(binary, "exp", x).double()
            d = (y / x.double().exp() - 1).abs()
            row += [(d / U).max().item(), (d / ((1 + x.double().abs()) * U)).max().item()]
        Z = probe(binary, "exp", xp).double().sum(1).float()
        e = (probe(binary, "log", Z).double() - Z.double().log()).abs()
        kl = (e / ((1 + Z.double().log().abs()) * U)).max().item()
        print(f"N={N:4d} D={D:4d} K={K:5d}  codes: |x| <= {xe.abs().max().item():5.2f}  |δ| <= {row[0]:6.3f} u = {row[1]:.4f}·(1 + |x|)·u"
              f"   softmax: |x| <= {xp.abs().max().item():5.2f}  |δ| <= {row[2]:6.3f} u = {row[3]:.4f}·(1 + |x|)·u"
              f"   log Z in [{Z.log().min().item():.2f}, {Z.log().max().item():.2f}]: |ε| <= {kl:.4f}·(1 + |log Z|)·u", flush=True)
        worst = [max(worst[0], row[0], row[2]), max(worst[1], row[1], row[3]), max(worst[2], kl)]
    print(f"worst: __expf |δ| <= {worst[0]:.3f} u = {worst[1]:.4f}·(1 + |x|)·u   __logf |ε| <= {worst[2]:.4f}·(1 + |log l|)·u")


if __name__ == "__main__":
    main()
