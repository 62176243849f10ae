"""CPU: the Gaussian-blur augmentation stage. The torch ``augment_reference`` against the
independent fp64 oracle of tests/blur_oracle.py on every case the GPU tests run, the
conditions those cases rely on, the draw order, config validation, the flags, a tiny training
run, and the LDS plan arithmetic (csrc/include/blur_plan.h) under sanitizers."""
import dataclasses
import datetime
import os
import subprocess

import numpy as np
import pytest
import torch

import aug_oracle as O
import blur_oracle as BO
from simclr_pytorch_distributed_amd.config import parse_pretrain
from simclr_pytorch_distributed_amd.data import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_conditions():
    """What the other tests (here and on the GPU) rely on, before anything uses it."""
    assert A.blur_auto_kernel(32) == 3 and A.blur_auto_kernel(224) == 23
    assert BO.get_case("blur_8_k3")["cfg"].blur_k == 3
    assert BO.get_case("blur_ragged")["cfg"].blur_k == 3
    big = BO.get_case("blur_224_k23")
    assert big["cfg"].blur_k == 23 and big["cfg"].size == 224 and big["cfg"].n_views == 2
    plan = A.blur_plan(224)
    assert plan["lds_bytes"] > 64 * 1024 and plan["n_strips"] == 1      # above the default dynamic-LDS limit
    # blur_strips: more than one column strip with a partial last one, at the automatic rows per
    # round and at the explicit ones the GPU tests pass; every tap of the halo carries weight
    st = BO.get_case("blur_strips")["cfg"]
    assert st.size == 215 and st.blur_k == 63
    for rows in (0, 1, 3):
        plan = A.blur_plan(st.size, st.blur_k, rows)
        assert plan["n_strips"] > 1 and st.size % plan["strip"] != 0 and plan["strip"] + st.blur_k - 1 < st.size
    assert BO.weights(63, st.blur_sigma[0])[0] > 1e-7
    assert 224 * 3 > 256                                                 # a row is wider than the workgroup
    rm = BO.get_case("blur_reflect_max")["cfg"]
    assert (rm.blur_k - 1) // 2 == rm.size - 1
    for r in BO.get_case("blur_reflect_max")["rows"]:
        assert 1.5 <= r["p"]["sigma"] <= 2.0
    tiny = BO.weights(7, 0.1)
    assert tiny[3] == 1.0 and tiny[2] < 1e-21 and np.float32(np.exp(-0.5 * (2 / 0.1) ** 2)) == 0.0
    assert all(r["p"]["sigma"] == pytest.approx(0.1) for r in BO.get_case("blur_sigma_tiny")["rows"])
    odd = BO.get_case("blur_odd_row")
    assert odd["cfg"].n_views == 3 and odd["cfg"].size == 7 and len(odd["rows"]) == 15
    for name in BO.CASES:
        case = BO.get_case(name)
        rows = case["rows"]
        assert len(rows) <= 64
        assert sum(r["fragile"] for r in rows) <= 0.05 * len(rows), name
        if name != "blur_simclr_32":
            assert all(r["p"]["blur"] for r in rows), name
        lo, hi = case["cfg"].blur_sigma
        assert all(lo <= r["p"]["sigma"] <= hi for r in rows)
    mixed = [r["p"]["blur"] for r in BO.get_case("blur_simclr_32")["rows"]]
    assert len(mixed) == 64 and 0.25 * len(mixed) <= sum(mixed) <= 0.75 * len(mixed)


def test_oracle_blur_properties():
    """The oracle against its definition: a constant image is a fixed point, the weights sum
    to 1 and are symmetric, and an impulse next to the edge shows the reflection (the edge pixel
    is not repeated: the column at distance 1 behind the edge comes back, not the edge)."""
    w = BO.weights(5, 1.0)
    assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, w[::-1], rtol=0, atol=0)
    assert np.allclose(w / w[2], np.exp(-0.5 * np.arange(-2, 3) ** 2.0), rtol=1e-15)
    assert np.abs(BO.gaussian_blur(np.full((6, 6, 3), 0.25), 5, 1.3) - 0.25).max() < 1e-15
    assert BO.reflect_index(-2, 7, 5).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    img = np.zeros((5, 5, 3))
    img[2, 1] = 1.0
    out = BO.gaussian_blur(img, 3, 1.0)[2, :, 0]
    w3 = BO.weights(3, 1.0)
    # column 0 sees columns (1, 0, 1): the impulse twice
    assert np.allclose(out, w3[1] * np.array([2 * w3[0], w3[1], w3[0], 0, 0]), rtol=1e-14, atol=0)


_dev = {}


def _reference_colour_dev(name):
    """|augment_reference - oracle| per view in pre-normalise colour units, fragile views 0
    (computed once per case)."""
    if name not in _dev:
        case = BO.get_case(name)
        ref = A.augment_reference(case["data"], case["idx"], case["cfg"], case["seed"], case["offs"], case["hw"])
        assert ref.shape == (case["norm"].shape[0], case["cfg"].size, case["cfg"].size, 8)
        assert torch.all(ref[..., 3:] == 0)
        dev = np.abs(ref[..., :3].double().numpy() - case["norm"]) * np.asarray(case["cfg"].std)
        dev = dev.reshape(dev.shape[0], -1).max(1)
        _dev[name] = dev * np.array([not r["fragile"] for r in case["rows"]])
    return _dev[name]


@pytest.mark.parametrize("name", BO.CASES)
def test_reference_matches_oracle(name):
    dev = _reference_colour_dev(name)
    print(f"{name}: worst |augment_reference - oracle| = {dev.max():.3e} colour units "
          f"(floor of the case {BO.eps_ref(name):.1e}, EPS_BLUR_REF {BO.EPS_BLUR_REF:.1e})")
    assert dev.max() <= BO.eps_ref(name) <= BO.EPS_BLUR_REF, (name, dev)


def test_eps_blur_ref_is_the_measured_worst():
    """EPS_BLUR_REF is a measurement (rounded up to two digits), not a margin: the worst case
    reaches at least half of it."""
    worst = max(_reference_colour_dev(n).max() for n in BO.CASES)
    print(f"EPS_BLUR_REF measured {worst:.3e}, stored {BO.EPS_BLUR_REF:.3e}")
    assert 0.5 * BO.EPS_BLUR_REF <= worst <= BO.EPS_BLUR_REF
    rest = max(_reference_colour_dev(n).max() for n in BO.CASES if BO.eps_ref(n) != BO.EPS_BLUR_REF)
    print(f"EPS_BLUR_REF_REST measured {rest:.3e}, stored {BO.EPS_BLUR_REF_REST:.3e}")
    assert 0.5 * BO.EPS_BLUR_REF_REST <= rest <= BO.EPS_BLUR_REF_REST


def test_blur_off_is_bit_equal_to_a_config_without_the_fields():
    case = O.get_case("crop_standard")
    ref = A.augment_reference(case["data"], case["idx"], case["cfg"], case["seed"])
    assert case["cfg"].blur_p == 0.0 and case["cfg"].blur_kernel == 0 and tuple(case["cfg"].blur_sigma) == (0.1, 2.0)
    # the other blur fields are ignored (not even validated) while blur_p is 0
    off = dataclasses.replace(case["cfg"], blur_p=0.0, blur_kernel=8, blur_sigma=(0.5, 0.7))
    assert torch.equal(A.augment_reference(case["data"], case["idx"], off, case["seed"]), ref)
    on = dataclasses.replace(case["cfg"], blur_p=1.0)
    assert not torch.equal(A.augment_reference(case["data"], case["idx"], on, case["seed"]), ref)


def test_earlier_draws_do_not_depend_on_the_blur():
    base = A.AugConfig.simclr(32, O.MEAN, O.STD)
    on = A.AugConfig.simclr(32, O.MEAN, O.STD, blur_p=1.0)
    assert on.blur_p == 1.0 and base.blur_p == 0.0
    n_blur = 0
    for i in range(300):
        H, W = ((32, 32), (48, 64), (90, 40))[i % 3]
        key = O.view_key(11, i, i % 2, i % 64)
        p0 = A._view_params(base, H, W, A._Rng(key))
        p1 = A._view_params(on, H, W, A._Rng(key))
        assert set(p1) == set(p0) and {"blur", "sigma"} <= set(p1)
        for f in p0:
            if f != "blur":
                assert p0[f] == p1[f], f
        assert p1["blur"] is True and p0["blur"] is False and 0.1 <= p1["sigma"] <= 2.0
        half = A._view_params(dataclasses.replace(on, blur_p=0.5), H, W, A._Rng(key))
        n_blur += half["blur"]
    assert abs(n_blur / 300 - 0.5) <= 4 * (0.25 / 300) ** 0.5


@pytest.mark.parametrize("kw", [
    dict(size=32, blur_kernel=4),                      # even k
    dict(size=32, blur_kernel=1),                      # k = 1
    dict(size=5, blur_kernel=11),                      # r = 5 > S - 1 = 4
    dict(size=1),                                      # automatic k = 3 at S = 1
    dict(size=32, blur_sigma=(0.0, 1.0)),              # lo <= 0
    dict(size=32, blur_sigma=(-0.5, 1.0)),
    dict(size=32, blur_sigma=(1.5, 1.0)),              # lo > hi
    dict(size=256, blur_kernel=255),                   # no plan within 160 KiB
    dict(size=32, blur_p=1.5),
])
def test_invalid_configs_raise(kw):
    kw = dict(dict(blur_p=0.5), **kw)
    with pytest.raises(ValueError):
        A.AugConfig(**kw)


def test_plan_mirror():
    assert A.blur_plan(256, 255) is None and A.blur_plan(5, 9) is not None and A.blur_plan(5, 11) is None
    for S, k in ((32, 3), (224, 23), (96, 9), (512, 51), (300, 63)):
        plan = A.blur_plan(S, k)
        assert plan is not None and plan["lds_bytes"] + 256 <= 160 * 1024 and plan["strip"] * plan["n_strips"] >= S
    assert A.blur_plan(512)["n_strips"] == 2          # the ring of 51 rows of 512 pixels needs two strips
    A.AugConfig(size=5, blur_p=1.0, blur_kernel=9)    # r = S - 1 is valid


def test_flags_defaults_and_names_unchanged(tmp_path):
    now = datetime.datetime(2024, 1, 2, 3, 4)
    base = ["--model", "resnet18", "--synthetic", "--work_dir", str(tmp_path)]
    a = parse_pretrain(base, make_dirs=False, now=now)
    assert (a.blur_p, a.blur_kernel, tuple(a.blur_sigma)) == (0.0, 0, (0.1, 2.0))
    b = parse_pretrain(base + ["--blur_p", "0.5", "--blur_kernel", "5", "--blur_sigma", "0.2", "1.5"],
                       make_dirs=False, now=now)
    assert (b.blur_p, b.blur_kernel, tuple(b.blur_sigma)) == (0.5, 5, (0.2, 1.5))
    for f in ("model_name", "save_folder", "tb_folder"):
        assert getattr(a, f) == getattr(b, f)
    for bad in (["--blur_p", "1.5"], ["--blur_p", "-0.1"], ["--blur_sigma", "0", "1"], ["--blur_sigma", "2", "1"],
                ["--blur_kernel", "-3"]):
        with pytest.raises(ValueError):
            parse_pretrain(base + bad, make_dirs=False, now=now)


def test_tiny_pretrain_run_with_blur(tmp_path):
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.utils.tb import read_events
    opt = parse_pretrain(["--model", "resnet18", "--batch_size", "8", "--synthetic", "--synthetic_size", "32",
                          "--epochs", "1", "--max_steps", "2", "--backend", "torch", "--precision", "fp32",
                          "--learning_rate", "0.1", "--blur_p", "0.5", "--save_freq", "100", "--print_freq", "1",
                          "--work_dir", str(tmp_path / "ws")])
    eng = PretrainEngine(opt, device=torch.device("cpu"))
    assert eng.aug.blur_p == 0.5 and eng.aug.blur_k == 3 and tuple(eng.aug.blur_sigma) == (0.1, 2.0)
    x = eng.make_views(torch.arange(8), 1, 0)
    assert tuple(x.shape) == (16, 3, 32, 32) and torch.isfinite(x).all()
    path = eng.logger.path
    eng.run()
    assert eng.global_step == 2
    losses = [v for _, t, v in read_events(path) if t == "loss"]
    assert losses and all(np.isfinite(v) for v in losses)


def test_probe_and_knn_configs_never_blur():
    for cfg in (A.AugConfig.linear_train(32, O.MEAN, O.STD), A.AugConfig.evaluation(32, O.MEAN, O.STD)):
        assert cfg.blur_p == 0.0
        for b in range(200):
            assert not A._view_params(cfg, 32, 32, A._Rng(O.view_key(5, b, 0, b)))["blur"]


@pytest.fixture(scope="module")
def plan_check_exe(tmp_path_factory):
    """csrc/tools/blur_plan_check.cpp as a stand-alone program built with AddressSanitizer +
    UndefinedBehaviorSanitizer (compiled once for the tests below)."""
    exe = str(tmp_path_factory.mktemp("blur_plan") / "blur_plan_check")
    src = os.path.join(ROOT, "csrc", "tools", "blur_plan_check.cpp")
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                        f"-I{os.path.join(ROOT, 'csrc', 'include')}", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_plan_arithmetic_under_sanitizers(plan_check_exe):
    """The launcher's and binding's size arithmetic (csrc/include/blur_plan.h) under the
    sanitizers: the sweep, and the simulated addressing of the kernel."""
    r = subprocess.run([plan_check_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "BLUR-PLAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_python_plan_mirror_equals_the_header_over_the_sweep(plan_check_exe):
    """data/augment.py blur_plan() is a second copy of blur_plan.h make_plan (AugConfig's
    ValueError must agree with the binding's TORCH_CHECK): every request of the sweep, S in
    1..512, k in 0..63 (0 = automatic), automatic and explicit rows, gives the same plan or the
    same refusal."""
    r = subprocess.run([plan_check_exe, "--table"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 512 * 64 * 4
    n_plans = n_strips = 0
    for line in lines:
        req, got = line.split(" -> ")
        S, k, rows = (int(x) for x in req.split())
        plan = A.blur_plan(S, k, rows)
        want = "none" if plan is None else " ".join(str(plan[f]) for f in ("k", "rows", "strip", "n_strips", "lds_bytes"))
        assert got == want, (line, plan)
        n_plans += plan is not None
        n_strips += plan is not None and plan["n_strips"] > 1
    print(f"{len(lines)} requests, {n_plans} plans, {n_strips} of them in strips")
    # both outcomes and the strip path are in the sweep
    assert n_plans > 50000 and len(lines) - n_plans > 50000 and n_strips > 1000
