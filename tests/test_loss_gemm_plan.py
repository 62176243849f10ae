"""Tile maps of the two-view loss GEMMs (host-only, CPU): the grouped tile walk that bt_xcorr, bt_bwd,
vic_bwd and vic_cov share and the triangle fold that decides where every vic_cov workgroup writes
(csrc/include/loss_gemm_plan.h), enumerated by a stand-alone program. No kernel runs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_and_fold_under_sanitizers(tmp_path):
    """For T = 1…64 and D = 64, 192, 320 the fold visits each (ti, tj), ti <= tj, exactly once and
    nothing else, fold_w·fold_h = tiles; for 1…17 x 1…9 grids the walk by groups of 4 is a bijection
    that goes down a tile column inside a group. Built with AddressSanitizer +
    UndefinedBehaviorSanitizer: a tile outside its grid is a heap overflow of the visit counts."""
    exe = str(tmp_path / "loss_gemm_plan_check")
    src = os.path.join(ROOT, "csrc", "tools", "loss_gemm_plan_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        f"-I{os.path.join(ROOT, 'csrc', 'include')}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOSS-GEMM-PLAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
