"""The MFMA classifier head's specification on the CPU: the twin of the kernels' arithmetic
(headgemm_checks.Twin, tiled from the Python mirror of the plan) passes every check that the GPU
test applies to the kernels, every named defect injected into it is caught, the plan header holds
its invariants under the sanitizers and matches the mirror, and the flag parses."""
import os
import subprocess

import pytest
import torch

import headgemm_checks as CK
import headgemm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", CK.case_names())
def test_twin_passes_every_check(name):
    c = CK.case(name)
    worst = CK.Worst()
    twin = CK.Twin()
    CK.run_steps(twin, c, worst, vs_exact=True)
    CK.run_ce(twin, c, worst, vs_exact=True)
    print(f"{name}: worst error/bound  {worst.report()}")


def _caught(defect, name):
    c = CK.case(name)
    twin = CK.Twin(defect)
    hits = []
    for run in (CK.run_steps, CK.run_ce):
        try:
            run(twin, c, None, vs_exact=True)
        except AssertionError as e:
            hits.append(str(e)[:120])
    return hits


@pytest.mark.parametrize("defect", CK.DEFECTS)
def test_every_defect_is_caught(defect):
    # G = 3 (head indices, the sweep layout), B = 31 and C = 17 (both reduction tails), a tie at
    # the label of row 0, garbage momentum at the first step, non-zero sinks, gout = 1.7
    hits = _caught(defect, "g3_b31_c17")
    if not hits:
        # (an fp32 sum of 31 rows can round to the fp64 sum's fp32 value: 65 rows as well)
        hits = _caught(defect, "g3_b65_k192_c17") + _caught(defect, "b65_c64")
    assert hits, f"defect {defect} passed every check"
    print(f"{defect}: {hits[0]}")


def test_single_bf16_exceeds_the_bound_by_a_wide_factor():
    """The cases are sized so that one bf16 product per element (no lo terms) misses the
    split-vs-exact budget by far more than a rounding's worth."""
    for name in ("g3_b31_c17", "b65_c64"):
        c = CK.case(name)
        G, C, K = c.W.shape
        P = O.plan(G, c.B, K, C)
        z = CK.Twin("single_bf16").logits(c.x, c.W, c.b, P).double()
        Wf = c.W.reshape(G * C, K)
        shape = lambda t: t.reshape(c.B, G, C).permute(1, 0, 2)  # noqa: E731
        ze = shape(O.dense(c.x, Wf)) + c.b.double()[:, None, :]
        bound = shape(CK.gemm_bound1(c.x, Wf, K) + CK.gemm_bound2(c.x, Wf))
        ratio = float(((z - ze).abs() / bound).max())
        print(f"{name}: single-bf16 error / (B1 + B2) = {ratio:.1f}")
        assert ratio > 8.0


def test_bound2_is_the_three_eps_budget():
    c = CK.case("b33_k192_c63")
    Wf = c.W[0]
    b2 = CK.gemm_bound2(c.x, Wf)
    assert bool((b2 <= CK.SECOND_ORDER * CK.EPS3 * (c.x.double().abs() @ Wf.double().abs().t())).all())


def test_plan_checker_under_sanitizers_and_mirror(tmp_path):
    exe = str(tmp_path / "head_gemm_plan_check")
    src = os.path.join(ROOT, "csrc", "tools", "head_gemm_plan_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        f"-I{os.path.join(ROOT, 'csrc', 'include')}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HEAD-GEMM-PLAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    r = subprocess.run([exe, "--dump"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [[int(v) for v in line.split()] for line in r.stdout.splitlines() if line.strip()]
    assert len(rows) > 1000
    n_ok = 0
    for row in rows:
        assert row == O.plan_row(*row[:4]), row[:4]
        n_ok += row[4]
    assert 0 < n_ok < len(rows)          # both supported and refused cases were compared


def test_plan_is_independent_of_G():
    for B, K, C in ((31, 64, 17), (256, 2048, 1000)):
        one = O.plan(1, B, K, C)
        for G in (3, 16):
            p = O.plan(G, B, K, C)
            assert p["nn"] == one["nn"]
            for f in ("nt", "tn"):
                assert p[f]["chunks"] == one[f]["chunks"] and p[f]["red_pad"] == one[f]["red_pad"]
            assert p["nt"] == O.plan(1, B, K, G * C)["nt"]


def test_flag_parses_and_defaults_to_fma(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_ce, parse_linear
    base = ["--work_dir", str(tmp_path)]
    for parse in (parse_linear, parse_ce):
        assert parse(base, make_dirs=False).head_gemm == "fma"
        assert parse(base + ["--head_gemm", "mfma"], make_dirs=False).head_gemm == "mfma"
        assert parse(base + ["--head_gemm", "fma"], make_dirs=False).head_gemm == "fma"
        with pytest.raises(SystemExit):
            parse(base + ["--head_gemm", "auto"], make_dirs=False)


def test_supported_ranges():
    from simclr_pytorch_distributed_amd.ops import ce_head, linear_probe
    ok = linear_probe.shape_supported
    assert ok(192, 1030, "mfma") and ok(4096, 32768, "mfma") and ok(64, 1, "mfma")
    assert not ok(96, 10, "mfma") and not ok(64, 40000, "mfma") and not ok(4160, 10, "mfma")
    assert ok(2048, 1000) and not ok(192, 10) and not ok(2048, 1030)          # the fma range is unchanged
    with pytest.raises(ValueError):
        ok(64, 10, "auto")
    # no GPU tensor: neither path is "supported", whatever the shape
    fc = torch.nn.Linear(192, 1030)
    assert not ce_head.supported(fc, "mfma") and not ce_head.supported(fc)
    assert O.supported(1, 8, 192, 1030) and not O.supported(1, 8, 96, 10) and not O.supported(1, 8, 64, 40000)


def test_engines_fall_back_with_one_warning(tmp_path, caplog):
    """--head_gemm mfma where it cannot run (CPU): one warning line, then the path of today."""
    import logging
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    opt = parse_linear(["--work_dir", str(tmp_path), "--synthetic", "--synthetic_size", "64", "--model", "resnet18",
                        "--batch_size", "32", "--epochs", "1", "--backend", "torch", "--head_gemm", "mfma"])
    with caplog.at_level(logging.WARNING):
        eng = LinearEngine(opt, device=torch.device("cpu"))
    assert eng.head_gemm == "fma" and eng.native_ce is None
    assert sum("--head_gemm mfma cannot run" in r.getMessage() for r in caplog.records) == 1
