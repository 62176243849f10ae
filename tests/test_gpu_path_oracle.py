"""The kernels between the last conv and the contrastive loss against the fp64 oracle of
tests/path_oracle.py: global average pool (csrc/kernels/pool.hip), the projection head
(csrc/bindings/head_ops.cpp: cast, GEMMs with the bias / ReLU / fp32-store / masked-store
epilogues, bias-gradient reductions), row normalisation and norm statistics
(csrc/kernels/featnorm.hip). Cases, guard, derived bounds and comparisons: tests/path_checks.py;
tests/test_path_oracle.py shows on the CPU that the comparisons catch each defect they are meant
for and that each case sits on the path it is named for.

Observed on one MI355X (the whole file: 44 tests, 17.5 s; slowest: each pinned-tile child process,
2.2 s; the 4100 x 2048 pool case 0.85 s, the 64 x 2048 x 2048 head case 0.4 s):
  bit-equal, zero tolerance: every head quantity (fb, h, z, dfeat, dW1, db1, dW2, db2 after one
    and two passes) in all 7 cases x 2 regimes, on the side stream, from a bf16 feat, through
    projection_head, and at 2056 rows on tile configs 0, 1, 2, 3 (auto), 4 and 6; gap_bwd in all
    5 cases x 2 regimes; gap_fwd in the exact regime of all 5 cases. No case was refused: the
    72 -> 136 -> 24 head runs.
  largest error / bound of the bounded quantities: gap_fwd (random bf16) 0.034; rownorm norms
    0.35, y 0.38, dx judged alone 0.18, dx chained 0.12; norm_stats Σ‖x‖ 0.10, Σ‖x‖² 0.10, mean
    0.22, var 0.045, rec 0.22, loss_sec 0.12, loss_l2 0.12; two-rank loss_sec 0.026, loss_l2 0.067.
    These are the CPU twin's ratios to every printed digit: the twin reproduces the kernels'
    summation orders.
No defect was found in the kernels or bindings.
"""
import os
import subprocess
import sys

import pytest
import torch

import path_checks as K
import path_oracle as O

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error / bound:", {k: f"{v:.3g}" for k, v in K.RATIO.items()})


# ---------------------------------------------------------------- projection head --------------

@pytest.mark.parametrize("name", list(K.HEAD_CASES))
def test_head(impl, name):
    """head_fwd / head_bwd on raw tensors, both regimes, bit for bit: fb, h, z, dfeat and the four
    sinks (views in a sentinel buffer) after one and two passes; side = 0 and the side stream, a
    bf16 feat and a second run give the same bits."""
    assert set(K.head_cfgs(impl.m, name).values()) == {3}
    for regime in K.REGIMES:
        K.check_head_behaviour(impl, name, regime)


@pytest.mark.parametrize("cfg", K.CHILD_CFGS)
def test_head_above_2048_rows_on_pinned_tiles(gpu, cfg):
    """Above 2048 rows head_cfg() asks auto_cfg; SDX_CONV_CFG (read once per process) pins that
    choice, so one fresh child per tile config runs the 2056-row case: the bias + ReLU forward, the
    fp32-store forward and the fp32-store data gradient on that tile, the masked data gradient on
    64 x 64. The child asserts the configs through conv_plan."""
    e = dict(os.environ, SDX_AUTOBUILD="0", PYTHONPATH=os.pathsep.join([ROOT, TESTS]), SDX_CONV_CFG=str(cfg))
    r = subprocess.run([sys.executable, os.path.join(TESTS, "path_checks.py"), "--child", str(cfg)], env=e,
                       capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and K.CHILD_MARKER in r.stdout, (cfg, r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("name", ["two M-tiles, 8 K-tiles", "linear"])
def test_projection_head_module_gives_the_raw_calls_bits(gpu, name):
    """ops.head.projection_head with a ConvWeightCache (bf16 weights in both layouts, gradients
    into param.grad, the side-stream join at the end of backward): the oracle's bits."""
    import torch.nn as nn
    from simclr_pytorch_distributed_amd.ops.head import projection_head
    from simclr_pytorch_distributed_amd.ops.weights import ConvWeightCache
    rows, D, O1, O2, _ = K.HEAD_CASES[name]
    for regime in K.REGIMES:
        d, r = K.head_inputs(name, regime), K.head_ref(name, regime)
        mod = nn.Sequential(nn.Linear(D, O1), nn.ReLU(inplace=True), nn.Linear(O1, O2)) if O2 else nn.Linear(D, O1)
        lins = [x for x in mod.modules() if isinstance(x, nn.Linear)]
        with torch.no_grad():
            for lin, w, b in zip(lins, ("w1", "w2"), ("b1", "b2")):
                lin.weight.copy_(d[w])
                lin.bias.copy_(d[b])
        mod = mod.to(gpu)
        wc = ConvWeightCache(lins, None)
        wc.refresh()
        feat = d["feat"].to(F32).to(gpu).requires_grad_(True)
        z = projection_head(feat, mod, wc)
        z.backward(d["dz"].to(F32).to(gpu))
        ctx = f"(projection_head '{name}' {regime})"
        K.same("z", z.detach().cpu().to(F64), r["f"]["z"], ctx)
        K.same("dfeat", feat.grad.cpu().to(F64), r["b"]["dfeat"], ctx)
        want = [r["b"]["dw1"], r["b"]["db1"] if O2 else r["b"]["db_last"]] + ([r["b"]["dw2"], r["b"]["db_last"]] if O2 else [])
        for (n, p), g in zip(mod.named_parameters(), want):
            K.same(n + ".grad", p.grad.cpu().to(F64), g, ctx)


# ---------------------------------------------------------------- global average pool ----------

@pytest.mark.parametrize("case", K.GAP_CASES)
def test_gap(impl, case):
    for regime in K.GAP_REGIMES:
        K.check_gap(impl, case, regime)


def test_gap_autograd_wrapper_with_a_bf16_upstream_gradient(impl, gpu):
    from simclr_pytorch_distributed_amd.ops.pool import global_avgpool_nhwc
    case = K.GAP_CASES[3]
    N, H, W, C = case
    d = K.gap_inputs(case, "wide")
    x = d["x"].to(BF16).to(gpu).requires_grad_(True)
    y = global_avgpool_nhwc(x)
    assert y.dtype == F32 and torch.equal(y.detach(), impl.m.gap_fwd(x.detach()))
    g16 = d["dy"].to(BF16).to(gpu)
    y.to(BF16).backward(g16)
    assert x.grad.dtype == BF16 and torch.equal(x.grad, impl.m.gap_bwd(g16.float(), H, W))
    K.same("dx", x.grad.cpu().to(F64), O.gap_bwd(g16.cpu().to(F64), H, W), f"(gap autograd {case})")


# ---------------------------------------------------------------- row normalisation ------------

@pytest.mark.parametrize("D", K.ROWNORM_D)
def test_rownorm(impl, D):
    for N in K.ROWNORM_N:
        K.check_rownorm(impl, N, D)


def test_rownorm_refuses_257_columns(impl, gpu):
    x = torch.randn(4, 257, device=gpu)
    with pytest.raises(RuntimeError):
        impl.m.rownorm_fwd(x, K.EPS)


# ---------------------------------------------------------------- norm statistics --------------

@pytest.mark.parametrize("D", K.STATS_D)
def test_norm_stats(impl, D):
    """Modes 0 / 1 / 2 over three steps of one in-place state, random and equal-norm rows; D % 4
    != 0 runs the scalar loads."""
    for N in K.STATS_N:
        for kind in ("random", "equal"):
            K.check_norm_stats(impl, N, D, kind, 0.9)


@pytest.mark.parametrize("momentum", [1.0, 0.1])
def test_norm_stats_momenta(impl, momentum):
    for N, D in ((65, 100), (300, 102), (257, 4)):
        for kind in ("random", "equal"):
            K.check_norm_stats(impl, N, D, kind, momentum)


def test_norm_stats_two_ranks(impl):
    for N, D in ((1, 3), (65, 100), (300, 102), (257, 128)):
        for kind in ("random", "equal"):
            K.check_norm_stats_two_ranks(impl, N, D, kind)
