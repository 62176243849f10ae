"""CPU: the torch ``augment_reference`` (the CPU training path, and the GPU kernel's twin)
against the independent fp64 oracle of tests/aug_oracle.py on every case the GPU tests run,
and the statistical / structural properties of the draw function ``_view_params``."""
import itertools
import math

import numpy as np
import pytest
import torch

import aug_oracle as O
from simclr_pytorch_distributed_amd.data import augment as A


_dev = {}


def _reference_colour_dev(case):
    """|augment_reference - oracle| per view in pre-normalise colour units, fragile views 0
    (computed once per case)."""
    if case["name"] not in _dev:
        _dev[case["name"]] = _measure(case)
    return _dev[case["name"]]


def _measure(case):
    ref = A.augment_reference(case["data"], case["idx"], case["cfg"], case["seed"], case["offs"], case["hw"])
    assert ref.shape == (case["norm"].shape[0], case["cfg"].size, case["cfg"].size, 8)
    assert torch.all(ref[..., 3:] == 0)
    dev = np.abs(ref[..., :3].double().numpy() - case["norm"]) * np.asarray(case["cfg"].std)
    dev = dev.reshape(dev.shape[0], -1).max(1)
    keep = np.array([not r["fragile"] for r in case["rows"]])
    return dev * keep


@pytest.mark.parametrize("name", O.CASES)
def test_reference_matches_oracle(name):
    case = O.get_case(name)
    dev = _reference_colour_dev(case)
    print(f"{name}: worst |augment_reference - oracle| = {dev.max():.3e} colour units (EPS_REF {O.EPS_REF:.1e})")
    assert dev.max() <= O.EPS_REF, (name, dev)


def test_eps_ref_is_the_measured_worst():
    """EPS_REF is a measurement (rounded up to two digits), not a margin: the worst case
    reaches at least half of it."""
    worst = max(_reference_colour_dev(O.get_case(n)).max() for n in O.CASES)
    print(f"EPS_REF measured {worst:.3e}, stored {O.EPS_REF:.3e}")
    assert 0.5 * O.EPS_REF <= worst <= O.EPS_REF


# ---- the conditions the GPU tests rely on, asserted here where no GPU is needed -----------

def test_identity_is_the_normalised_source_view_major():
    for nv in (1, 2, 3):
        case = O.get_case(f"identity_v{nv}")
        B = len(case["idx"])
        assert case["norm"].shape[0] == nv * B
        for v in range(nv):
            for b in range(B):
                src = case["data"][int(case["idx"][b])].double().numpy() / 255.0
                want = (src - np.asarray(O.MEAN)) / np.asarray(O.STD)
                assert np.abs(case["norm"][v * B + b] - want).max() < 1e-14


def test_case_conditions():
    flips = [r["p"]["flip"] for r in O.get_case("flip_only")["rows"]]
    assert any(flips) and not all(flips)
    full = O.get_case("jitter_full")
    assert len(full["rows"]) <= 64 and all(r["p"]["jitter"] for r in full["rows"])
    assert {tuple(r["p"]["order"]) for r in full["rows"]} == set(itertools.permutations(range(4)))
    for name in ("jitter_brightness", "jitter_contrast", "jitter_saturation", "jitter_hue", "jitter_hue_wide",
                 "gray_jitter"):
        assert all(r["p"]["jitter"] for r in O.get_case(name)["rows"])
    assert all(r["p"]["gray"] for r in O.get_case("gray_only")["rows"] + O.get_case("gray_jitter")["rows"])
    # brightness really clamps somewhere on the palette
    assert max(r["p"]["fb"] for r in O.get_case("jitter_brightness")["rows"]) > 1.3
    for name in O.CASES:
        rows = O.get_case(name)["rows"]
        assert len(rows) <= 64
        assert sum(r["fragile"] for r in rows) <= 0.05 * len(rows), name
    # scale=(0.9, 1): rejected tries advance the draw counter
    assert max(r["tries"] for r in O.get_case("crop_high_scale")["rows"]) >= 3
    fb = O.get_case("crop_fallback")
    boxes = {}
    for r in fb["rows"]:
        boxes.setdefault(r["img"].shape[:2], []).append((r["box"], r["fallback"]))
    assert all(b == ((0, 18, 40, 53), True) for b in boxes[(40, 90)])      # ratio clamped from above
    assert all(b == ((18, 0, 53, 40), True) for b in boxes[(90, 40)])      # ... from below
    assert all(b[0] == (0, 0, 33, 33) for b in boxes[(33, 33)])
    assert any(b[1] for b in boxes[(33, 33)])                              # the in-range branch


# ---- properties of the draws --------------------------------------------------------------

def test_uni_range():
    rng = A._Rng(12345)
    u = np.array([rng.uni() for _ in range(20000)])
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 4 * math.sqrt(1 / 12 / len(u))


def test_view_params_properties():
    cfg = A.AugConfig.simclr(32, O.MEAN, O.STD)
    N = 20000
    flips = jit = gray = 0
    orders = set()
    for i in range(N):
        H, W = ((32, 32), (48, 64), (90, 40), (57, 71))[i % 4]
        key = O.view_key(11, i, i % 2, i % 64)
        p = A._view_params(cfg, H, W, A._Rng(key))
        ci, cj, ch, cw = p["ci"], p["cj"], p["ch"], p["cw"]
        assert ci == int(ci) and cj == int(cj) and ch == int(ch) and cw == int(cw)
        assert 0 <= ci and 0 <= cj and ch >= 1 and cw >= 1 and ci + ch <= H and cj + cw <= W
        box, fragile, fallback, _ = O.redraw_crop(cfg, H, W, key)
        if not fragile:
            assert box == (ci, cj, ch, cw)
        if not fallback:
            # w = rint(sqrt(t*ar)), h = rint(sqrt(t/ar)), t/(H*W) in scale, ar in ratio
            assert (cw - 0.5) * (ch - 0.5) <= cfg.scale[1] * H * W * (1 + 1e-6)
            assert (cw + 0.5) * (ch + 0.5) >= cfg.scale[0] * H * W * (1 - 1e-6)
            assert (cw - 0.5) / (ch + 0.5) <= cfg.ratio[1] * (1 + 1e-6)
            assert (cw + 0.5) / (ch - 0.5) >= cfg.ratio[0] * (1 - 1e-6)
        for f, s in ((p["fb"], cfg.brightness), (p["fc"], cfg.contrast), (p["fs"], cfg.saturation)):
            assert 1 - s <= f <= 1 + s
        assert -cfg.hue <= p["fh"] <= cfg.hue
        assert sorted(p["order"]) == [0, 1, 2, 3]
        flips += p["flip"]
        jit += p["jitter"]
        gray += p["gray"]
        orders.add(tuple(p["order"]))
    for count, prob in ((flips, 0.5), (jit, 0.8), (gray, 0.2)):
        assert abs(count / N - prob) <= 4 * math.sqrt(prob * (1 - prob) / N), (count, prob)
    assert len(orders) == 24


def test_two_views_of_a_sample_differ_and_probe_configs_never_jitter():
    cfg = A.AugConfig.simclr(32, O.MEAN, O.STD)
    for b in range(50):
        a, c = (A._view_params(cfg, 32, 32, A._Rng(O.view_key(5, 7 * b, v, b))) for v in (0, 1))
        assert a != c
    for cfg in (A.AugConfig.linear_train(32, O.MEAN, O.STD), A.AugConfig.evaluation(32, O.MEAN, O.STD)):
        assert cfg.n_views == 1
        for b in range(500):
            p = A._view_params(cfg, 32, 32, A._Rng(O.view_key(5, b, 0, b)))
            assert not p["jitter"] and not p["gray"]
            if not cfg.crop:
                assert (p["ci"], p["cj"], p["ch"], p["cw"], p["flip"]) == (0, 0, 32, 32, False)
