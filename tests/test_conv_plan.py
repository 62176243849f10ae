"""Conv dispatch plan (host-only, CPU): which tile config auto dispatch gives every stride-1
3x3 conv of the two benchmark configs, and how many statistics-slab rows its launch writes.

Covers the padded-row tap-reuse tiles (conv_plan.h tap_geom t_rw): at 56x56 (224x224 config,
stage 1) a 256-row tile holds 4 image rows of 64 virtual pixels (56 real), so the slab has
N*H*64/256 rows, not ceil(N*H*W/256). The plan is computed by the extension's host code
only (`conv_plan`), no kernel runs.
"""
import json
import os
import subprocess
import sys

import pytest

from simclr_pytorch_distributed_amd.ops import _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.json")


@pytest.fixture(scope="module")
def m():
    mod = _ext.ext()
    if mod is None or not hasattr(mod, "conv_plan"):
        pytest.skip("native extension not built")
    return mod


# (N, H, C, K) -> expected tap cfg of the fwd and of the dgrad (both stride-1 3x3, pad 1)
CIFAR = [
    ((512, 32, 64, 64), 11),     # bands of 8 image rows
    ((512, 16, 128, 128), 12),   # one image per 256-row tile
    ((512, 8, 256, 256), 12),    # 4 images per tile
    ((512, 4, 512, 512), 13),    # 8 images per 128-row tile
]


@pytest.mark.parametrize("shape,cfg", CIFAR)
def test_cifar_3x3_on_tap_tiles(m, shape, cfg):
    N, H, C, K = shape
    bm = {11: 256, 12: 256, 13: 128}[cfg]
    for dgrad in (False, True):
        got_cfg, mt = m.conv_plan(N, H, H, C, K, 3, 3, 1, 1, dgrad)
        assert got_cfg == cfg
        assert mt == (N * H * H + bm - 1) // bm   # unpadded: whole images / bands


def test_56x56_padded_rows(m):
    N = 1024
    for dgrad in (False, True):
        cfg, mt = m.conv_plan(N, 56, 56, 64, 64, 3, 3, 1, 1, dgrad)
        assert cfg == 11
        assert mt == N * 56 * 64 // 256            # virtual rows: 64 per image row
        assert mt != (N * 56 * 56 + 255) // 256


@pytest.mark.parametrize("H,C", [(28, 128), (14, 256), (7, 512)])
def test_no_tap_tile_where_it_loses_or_misfits(m, H, C):
    # 28x28: the padded 128-row tile loses to the implicit GEMM (profiles/tap_pad_r6.txt);
    # 14x14 / 7x7: no band of whole (padded) rows fits a tile
    cfg, mt = m.conv_plan(1024, H, H, C, C, 3, 3, 1, 1, False)
    assert cfg not in (11, 12, 13)
    bm = {0: 128, 1: 256, 2: 64, 3: 64, 4: 128, 5: 256, 6: 128}[cfg]
    assert mt == (1024 * H * H + bm - 1) // bm


def test_1x1_plan_is_implicit_gemm(m):
    cfg, mt = m.conv_plan(512, 32, 32, 256, 64, 1, 1, 1, 0, False)
    assert cfg not in (11, 12, 13) and mt > 0


# ---- the golden table: every fwd / dgrad / wgrad plan of the benchmark networks' convs and of
# the GPU tests' edge shapes, under the default knobs, each run-time setter and each env
# setting that tests or recipes use (tools/conv_plan_golden.py documents and records it)

def _compute_all(m, gold):
    """{"<shape index>/<request>": the plan's values of gold["fields"][kind]} for every table entry."""
    out = {}
    for i, (shape, plans) in enumerate(gold["shapes"]):
        N, H, W, C, K, R, S, st, pad = shape
        for name in plans:
            kind, in_bn, bnstat, cat_ch, splits, cfg, acc = gold["requests"][name]
            d = m.conv_plan(N, H, W, C, K, R, S, st, pad, kind == "dgrad", full=True, kind=kind, in_bn=bool(in_bn),
                            bnstat=bool(bnstat), cat_ch=C if cat_ch < 0 else cat_ch, splits=splits, cfg=cfg,
                            accumulate=bool(acc))
            assert d["ok"]
            out[f"{i}/{name}"] = [d[f] for f in gold["fields"][kind]]
    return out


def _diff(gold, name, rows):
    """Entries whose plan is not the default plan with the setting's recorded field changes."""
    over = gold["settings"][name] if name else {}
    bad = []
    for i, (shape, plans) in enumerate(gold["shapes"]):
        for req, base in plans.items():
            key = f"{i}/{req}"
            fields = gold["fields"][gold["requests"][req][0]]
            want = [over.get(key, {}).get(f, b) for f, b in zip(fields, base)]
            if rows[key] != want:
                bad.append((shape, req, dict(zip(fields, want)), dict(zip(fields, rows[key]))))
    return bad


SETTERS = {
    "tap3_set(0)": ("tap3_set", (0,), (1,)),
    "wgrad_block_target_set(256)": ("wgrad_block_target_set", (256,), (128,)),
    "wgrad1x1_big_set(0)": ("wgrad1x1_big_set", (0,), (1,)),
    "wgrad1x1_big_set(2)": ("wgrad1x1_big_set", (2,), (1,)),
    "wgrad1x1_pairs_set(1)": ("wgrad1x1_pairs_set", (1,), (0,)),
    "igemm_one_k_set(0,64)": ("igemm_one_k_set", (0, 64), (0, 256)),
    "igemm_one_k_set(1,256)": ("igemm_one_k_set", (1, 256), (1, 64)),
}


def test_golden_table_every_row_exact(m):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["shapes"]) > 100 and len(gold["settings"]) == len(SETTERS) + 6
    bad = {"default": _diff(gold, "", _compute_all(m, gold))}
    seen = {""}
    for name, (setter, args, restore) in SETTERS.items():
        prev = getattr(m, setter)(*args)
        try:
            assert prev == restore[-1], (name, prev)      # the documented default; setters return the previous value
            bad[name] = _diff(gold, name, _compute_all(m, gold))
        finally:
            assert getattr(m, setter)(*restore) == args[-1]
        seen.add(name)
    assert _diff(gold, "", _compute_all(m, gold)) == []   # every setter restored
    # env settings are read once per process: a fresh child each
    tool = os.path.join(ROOT, "tools", "conv_plan_golden.py")
    procs = {}
    for name in gold["settings"]:
        if name in seen:
            continue
        var, val = name.split("=")
        env = dict(os.environ)
        env[var] = val
        procs[name] = subprocess.Popen([sys.executable, tool, "--dump"], env=env, stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert len(procs) == 6
    for name, pr in procs.items():
        out, err = pr.communicate(json.dumps([s for s, _ in gold["shapes"]]), timeout=120)
        assert pr.returncode == 0, (name, err[-2000:])
        bad[name] = _diff(gold, name, json.loads(out))
    differing = {n: b[:3] for n, b in bad.items() if b}
    assert not differing, differing


def test_plan_invariants_under_sanitizers(tmp_path):
    """csrc/include/conv_plan.h in a stand-alone program built with AddressSanitizer +
    UndefinedBehaviorSanitizer: split ranges, slab sizes, 32-bit index ranges, halo reads."""
    exe = str(tmp_path / "conv_plan_check")
    src = os.path.join(ROOT, "csrc", "tools", "conv_plan_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        f"-I{os.path.join(ROOT, 'csrc', 'include')}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CONV-PLAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
