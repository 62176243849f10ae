"""CPU: the evaluation transform Resize + CenterCrop + normalize.

* the fp64 oracle of tests/evalcrop_oracle.py against torch's antialiased bilinear interpolate in
  float64, its integer windows against the floating-point definition, and the conditions the
  named cases rely on;
* the fp32 CPU twin (augment_reference) against the oracle: EPS_CROP_REF is its measured worst;
* configs, flags and a tiny end-to-end run of both engines on an ImageFolder (torch backend).
"""
import dataclasses
import datetime
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_oracle as O
import evalcrop_oracle as EO
from simclr_pytorch_distributed_amd.data import augment as A

MEAN_S, STD_S, make_image_folder = EO.MEAN_S, EO.STD_S, EO.make_image_folder


def _runs():
    return [(n, k, run) for n in EO.CASES for k, run in enumerate(EO.get_case(n))]


# ------------------------------------------------------------ the oracle itself ---------------

def _images(run):
    for s in sorted(set(int(i) for i in run["idx"])):
        yield s, O.image(run, s)


@pytest.mark.parametrize("name", EO.CASES)
def test_oracle_matches_torch_interpolate(name):
    """Resized image within 1e-9 (0-255 scale) of F.interpolate(bilinear, antialias) in float64;
    every integer window equals the floating-point definition's; offsets are torchvision's."""
    for run in EO.get_case(name):
        R, S = run["cfg"].resize, run["cfg"].size
        for s, img in _images(run):
            H, W = img.shape[:2]
            oh, ow = EO.resized_hw(H, W, R)
            assert min(oh, ow) == R and max(oh, ow) == int(R * max(H, W) / min(H, W))
            got = EO.resize(img, R)
            t = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1).unsqueeze(0)
            want = F.interpolate(t, size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)
            diff = np.abs(got - want[0].permute(1, 2, 0).numpy()).max()
            assert diff <= 1e-9, (name, s, diff)
            for n_in, n_out in ((H, oh), (W, ow)):
                scale = n_in / n_out
                sup = max(scale, 1.0)
                for i in range(n_out):
                    c = scale * (i + 0.5)
                    lo, hi = EO.window(n_in, n_out, i)
                    assert 0 <= lo < hi <= n_in
                    # a bound that falls exactly on an integer carries weight 0 on either side of
                    # it, so only there may the floating-point floor differ from the exact one
                    flo, fhi = max(0, math.floor(c - sup + 0.5)), min(n_in, math.floor(c + sup + 0.5))
                    assert (lo, hi) == (flo, fhi) or abs((c - sup + 0.5) - round(c - sup + 0.5)) < 1e-9 \
                        or abs((c + sup + 0.5) - round(c + sup + 0.5)) < 1e-9, (name, n_in, n_out, i)
            top, left = int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))
            assert (EO.crop_offset(oh - S), EO.crop_offset(ow - S)) == (top, left)
            assert (A.center_crop_offset(oh - S), A.center_crop_offset(ow - S)) == (top, left)
            assert A.resized_hw(H, W, R) == (oh, ow)
        for row, s in enumerate(run["idx"]):
            img = O.image(run, int(s))
            oh, ow = EO.resized_hw(img.shape[0], img.shape[1], R)
            assert run["offsets"][row] == (int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0)))


def _tap_counts(n_in, n_out):
    return [hi - lo for lo, hi in (EO.window(n_in, n_out, i) for i in range(n_out))]


def test_case_conditions():
    """What the named cases pin, asserted here so that the GPU test need not."""
    # down_*: scale 2.3125, 5-tap windows clipped at both borders
    for name, short_axis in (("down_landscape", 0), ("down_portrait", 1)):
        (run,) = EO.get_case(name)
        hw = tuple(int(v) for v in run["hw"][0])
        assert hw[short_axis] == 37 and hw[1 - short_axis] == 53 and 37 / 16 == 2.3125
        taps = _tap_counts(37, 16)
        assert max(taps) >= 5 and taps[0] < max(taps) and taps[-1] < max(taps)
        assert EO.window(37, 16, 0)[0] == 0 and EO.window(37, 16, 15)[1] == 37
    # odd_offsets: d = 3 -> 2, d = 1 -> 0, d = 5 -> 2
    runs = EO.get_case("odd_offsets")
    assert [(r["cfg"].resize, r["cfg"].size) for r in runs] == [(16, 13), (16, 15), (17, 12)]
    assert [r["offsets"][0][0] for r in runs] == [2, 0, 2]
    assert [EO.crop_offset(d) for d in (0, 1, 2, 3, 4, 5, 6, 7)] == [0, 0, 1, 2, 2, 2, 3, 4]
    # the long axis: 37x53 -> 16x22 (d = 9, 7) and 17x24 (d = 12)
    assert [r["offsets"][0][1] for r in runs] == [4, 4, 6]
    # identity: scale 1 on both axes: windows {i, i+1} with weights {1, 0}
    (run,) = EO.get_case("identity")
    assert EO.resized_hw(16, 23, 16) == (16, 23)
    for n in (16, 23):
        assert np.array_equal(EO.axis_weights(n, n), np.eye(n))
        assert _tap_counts(n, n) == [2] * (n - 1) + [1]
    img = O.image(run, 0)
    top, left = run["offsets"][0]
    assert np.array_equal(run["colour"][0] * 255.0, img[top:top + 16, left:left + 16].astype(np.float64))
    # upsample: 2-tap windows, the store is smaller than R
    assert EO.resized_hw(9, 12, 16) == (16, 21) and max(_tap_counts(9, 16)) == 2 and max(_tap_counts(12, 21)) == 2
    # extreme: scale 12.5 on both axes (2 support + 1 = 26; the window [c - 12, c + 13) of the
    # definition holds 25 taps) and a 25:1 aspect
    assert EO.resized_hw(200, 300, 16) == (16, 24) and 200 / 16 == 300 / 24 == 12.5
    assert max(_tap_counts(200, 16)) == max(_tap_counts(300, 24)) == 25
    assert EO.resized_hw(8, 200, 16) == (16, 400) and 200 / 8 == 25
    # dense: the non-ragged addressing; ragged_mix: every size above, repeats, 16 rows
    (run,) = EO.get_case("dense")
    assert run["offs"] is None and tuple(run["data"].shape) == (5, 32, 32, 3) and EO.resized_hw(32, 32, 37) == (37, 37)
    (run,) = EO.get_case("ragged_mix")
    idx = [int(i) for i in run["idx"]]
    assert len(idx) == 16 and set(idx) == set(range(len(EO.MIX))) and idx != sorted(idx)
    assert {(37, 53), (53, 37), (16, 23), (9, 12), (200, 300), (8, 200), (32, 32)} == set(EO.MIX)
    # imagenet: production geometry (the kernel's 24-row bands: nine and a partial one of 8 rows);
    # the third image is at scale 1 (as after an R-capped load)
    (run,) = EO.get_case("imagenet")
    assert (run["cfg"].resize, run["cfg"].size) == (256, 224)
    assert EO.resized_hw(500, 375, 256) == (341, 256) and EO.resized_hw(375, 500, 256) == (256, 341)
    assert EO.resized_hw(256, 341, 256) == (256, 341)
    assert run["offsets"] == [(58, 16), (16, 58), (16, 58)]
    img = O.image(run, 2)
    assert np.array_equal(run["colour"][2] * 255.0, img[16:240, 58:282].astype(np.float64))


# ------------------------------------------------------------ the fp32 CPU twin ---------------

_dev = {}


def _twin_dev(name, k):
    """worst |augment_reference - oracle| of a run in colour units (computed once)."""
    if (name, k) not in _dev:
        run = EO.get_case(name)[k]
        cfg = run["cfg"]
        ref = A.augment_reference(run["data"], run["idx"], cfg, 0, run["offs"], run["hw"])
        assert ref.shape == (len(run["idx"]), cfg.size, cfg.size, 8) and ref.dtype == torch.float32
        assert torch.all(ref[..., 3:] == 0)
        _dev[name, k] = float((np.abs(ref[..., :3].double().numpy() - run["norm"]) * np.asarray(cfg.std)).max())
    return _dev[name, k]


@pytest.mark.parametrize("name", EO.CASES)
def test_reference_matches_oracle(name):
    for k in range(len(EO.get_case(name))):
        dev = _twin_dev(name, k)
        print(f"{name}[{k}]: worst |augment_reference - oracle| = {dev:.3e} colour units "
              f"(EPS_CROP_REF {EO.EPS_CROP_REF:.1e})")
        assert dev <= EO.EPS_CROP_REF, (name, k, dev)


def test_eps_crop_ref_is_the_measured_worst():
    """EPS_CROP_REF is a measurement (rounded up to two digits), not a margin."""
    worst = max(_twin_dev(n, k) for n, k, _ in _runs())
    print(f"EPS_CROP_REF measured {worst:.3e}, stored {EO.EPS_CROP_REF:.3e}")
    assert 0.5 * EO.EPS_CROP_REF <= worst <= EO.EPS_CROP_REF


def test_twin_is_exact_at_scale_one():
    for name, row in (("identity", 0), ("imagenet", 2)):
        (run,) = EO.get_case(name)
        cfg = run["cfg"]
        img = torch.from_numpy(O.image(run, int(run["idx"][row])))
        top, left = run["offsets"][row]
        crop = img[top:top + cfg.size, left:left + cfg.size].contiguous().unsqueeze(0)
        one = torch.tensor([int(run["idx"][row])])
        got = A.augment_reference(run["data"], one, cfg, 0, run["offs"], run["hw"])
        want = A.augment_reference(crop, torch.zeros(1, dtype=torch.long), A.AugConfig.evaluation(cfg.size, cfg.mean, cfg.std), 0)
        assert torch.equal(got, want)


def test_augment_dispatches_to_the_twin_on_cpu():
    (run,) = EO.get_case("down_landscape")
    a = A.augment(run["data"], run["idx"], run["cfg"], 5, run["offs"], run["hw"])
    b = A.augment_reference(run["data"], run["idx"], run["cfg"], 0, run["offs"], run["hw"])
    assert torch.equal(a, b)


# ------------------------------------------------------------ configs -------------------------

def test_resize_zero_is_bit_equal_to_a_config_without_the_field():
    case = O.get_case("crop_standard")
    cfg = case["cfg"]
    assert cfg.resize == 0
    ref = A.augment_reference(case["data"], case["idx"], cfg, case["seed"])
    assert torch.equal(A.augment_reference(case["data"], case["idx"], dataclasses.replace(cfg, resize=0), case["seed"]), ref)
    for make in (A.AugConfig.linear_train, A.AugConfig.evaluation, A.AugConfig.simclr):
        assert make(32, O.MEAN, O.STD).resize == 0
    assert A.AugConfig().resize == 0
    ev = A.AugConfig.evaluation(8, O.MEAN, O.STD)
    ident = O.get_case("identity_v1")
    assert torch.equal(A.augment_reference(ident["data"], ident["idx"], ev, 0),
                       A.augment_reference(ident["data"], ident["idx"], dataclasses.replace(ev, resize=0), 0))


def test_center_crop_config_and_default_resize():
    c = A.AugConfig.center_crop(224, O.MEAN, O.STD)
    assert (c.resize, c.size, c.n_views, c.crop, c.flip, c.jitter_p, c.gray_p, c.blur_p) == (256, 224, 1, False, False, 0, 0, 0)
    assert A.AugConfig.center_crop(32, O.MEAN, O.STD).resize == 37
    assert A.AugConfig.center_crop(32, O.MEAN, O.STD, resize=40).resize == 40
    assert [A.default_resize(s) for s in (224, 32, 1)] == [256, 37, 1]


def test_invalid_configs_raise():
    good = A.AugConfig.center_crop(16, O.MEAN, O.STD, resize=18)
    for kw in (dict(resize=15), dict(n_views=2), dict(crop=True), dict(flip=True), dict(jitter_p=0.5),
               dict(gray_p=0.2), dict(blur_p=0.5), dict(resize=40000)):
        with pytest.raises(ValueError):
            dataclasses.replace(good, **kw)
    with pytest.raises(ValueError):
        A.AugConfig.center_crop(16, O.MEAN, O.STD, resize=8)
    dataclasses.replace(good, resize=16)     # S == R is legal


# ------------------------------------------------------------ flags ---------------------------

NOW = datetime.datetime(2024, 5, 6, 7, 8)


def _folder(root, classes):
    for c in classes:
        os.makedirs(os.path.join(root, c))
    return str(root)


def test_linear_flags(tmp_path):
    from simclr_pytorch_distributed_amd.config import DATASET_STATS, parse_linear
    for ds, ncls in (("cifar10", 10), ("cifar100", 100)):
        o = parse_linear(["--dataset", ds, "--work_dir", str(tmp_path)], make_dirs=False, now=NOW)
        assert (o.size, o.resize, o.val_folder, o.mean, o.std, o.n_cls) == (32, 0, None, None, None, ncls)
        assert (o.mean_t, o.std_t) == DATASET_STATS[ds]
        assert o.model_name == f"{ds}_resnet50_lr_0.1_decay_0_bsz_512"
        assert o.save_folder == os.path.join(str(tmp_path), f"{ds}_models", "classifier_0506_0708_" + o.model_name)
        assert o.tb_folder == os.path.join(str(tmp_path), f"{ds}_tensorboard", "classifier_0506_0708_" + o.model_name)
    tr, va = _folder(tmp_path / "tr", "abc"), _folder(tmp_path / "va", "abc")
    base = ["--dataset", "path", "--data_folder", tr, "--work_dir", str(tmp_path)]
    o = parse_linear(base + ["--val_folder", va, "--mean", MEAN_S, "--std", STD_S, "--size", "224"], make_dirs=False, now=NOW)
    assert (o.size, o.resize, o.n_cls) == (224, 0, 0) and o.mean_t == (0.5, 0.45, 0.4) and o.std_t == (0.25, 0.2, 0.22)
    for missing in (["--mean", MEAN_S, "--std", STD_S], ["--val_folder", va, "--std", STD_S],
                    ["--val_folder", va, "--mean", MEAN_S]):
        with pytest.raises(ValueError):
            parse_linear(base + missing, make_dirs=False, now=NOW)
    # --synthetic needs no validation folder
    parse_linear(base + ["--mean", MEAN_S, "--std", STD_S, "--synthetic"], make_dirs=False, now=NOW)
    other = _folder(tmp_path / "other", "abd")
    with pytest.raises(ValueError, match="classes"):
        parse_linear(base + ["--val_folder", other, "--mean", MEAN_S, "--std", STD_S], make_dirs=False, now=NOW)
    with pytest.raises(ValueError, match="resize"):
        parse_linear(base + ["--val_folder", va, "--mean", MEAN_S, "--std", STD_S, "--size", "64", "--resize", "32"],
                     make_dirs=False, now=NOW)


def test_pretrain_flags(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    tr, va = _folder(tmp_path / "tr", "abc"), _folder(tmp_path / "va", "abc")
    base = ["--dataset", "path", "--data_folder", tr, "--mean", MEAN_S, "--std", STD_S, "--work_dir", str(tmp_path)]
    plain = parse_pretrain(["--work_dir", str(tmp_path)], make_dirs=False, now=NOW)
    assert (plain.val_folder, plain.resize) == (None, 0)
    with pytest.raises(ValueError, match="validation split"):
        parse_pretrain(base + ["--knn_freq", "1"], make_dirs=False, now=NOW)
    o = parse_pretrain(base + ["--knn_freq", "1", "--val_folder", va], make_dirs=False, now=NOW)
    assert (o.knn_freq, o.val_folder, o.resize) == (1, va, 0)
    a = parse_pretrain(base, make_dirs=False, now=NOW)
    for f in ("model_name", "save_folder", "tb_folder"):
        assert getattr(a, f) == getattr(o, f)
    other = _folder(tmp_path / "other", "ab")
    with pytest.raises(ValueError, match="classes"):
        parse_pretrain(base + ["--knn_freq", "1", "--val_folder", other], make_dirs=False, now=NOW)


# ------------------------------------------------------------ end to end (CPU, torch backend) --

def test_linear_engine_on_an_image_folder(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    tr, va = make_image_folder(str(tmp_path / "data"))
    opt = parse_linear(["--dataset", "path", "--data_folder", tr, "--val_folder", va, "--mean", MEAN_S, "--std", STD_S,
                        "--size", "32", "--model", "resnet18", "--backend", "torch", "--precision", "fp32", "--knn",
                        "--knn_k", "5", "--epochs", "1", "--max_steps", "2", "--batch_size", "8", "--num_workers", "2",
                        "--work_dir", str(tmp_path / "ws")])
    eng = LinearEngine(opt, device=torch.device("cpu"))
    assert opt.n_cls == 3 and eng.classifier.fc.out_features == 3
    assert eng.aug_val.resize == 37 and eng.aug_val.size == 32 and eng.aug_train.resize == 0 and eng.aug_train.crop
    assert eng.train.offs is not None and eng.val.offs is not None and len(eng.val) == 12
    assert int(eng.val.hw.min()) <= 37        # the validation store is capped at the Resize target
    assert int(eng.val.hw.min(dim=1).values.max()) <= 37
    logged = {}
    log_value = eng.logger.log_value

    def record(tag, value, step):
        logged[tag] = value
        return log_value(tag, value, step)

    eng.logger.log_value = record
    best, best5 = eng.run()
    for tag in ("knn/val_acc1", "knn/val_acc5", "classifier/val_acc1", "classifier/train_loss", "classifier/val_loss"):
        assert tag in logged, tag
        assert math.isfinite(logged[tag])
    for tag in ("knn/val_acc1", "knn/val_acc5", "classifier/val_acc1"):
        assert 0.0 <= logged[tag] <= 100.0
    assert 0.0 <= best <= 100.0 and 0.0 <= best5 <= 100.0


def test_pretrain_knn_bank_is_the_resident_store(tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    tr, va = make_image_folder(str(tmp_path / "data"))
    opt = parse_pretrain(["--dataset", "path", "--data_folder", tr, "--val_folder", va, "--mean", MEAN_S, "--std", STD_S,
                          "--size", "32", "--model", "resnet18", "--backend", "torch", "--precision", "fp32",
                          "--knn_freq", "1", "--knn_k", "5", "--epochs", "1", "--max_steps", "2", "--batch_size", "8",
                          "--num_workers", "2", "--learning_rate", "0.05", "--work_dir", str(tmp_path / "ws")])
    eng = PretrainEngine(opt, device=torch.device("cpu"))
    ev = eng.knn
    assert ev is not None and ev.n_cls == 3 and ev.aug.resize == 37
    assert ev.bank is eng.train and ev.bank.images.untyped_storage().data_ptr() == eng.train.images.untyped_storage().data_ptr()
    assert ev.bank.offs is eng.train.offs and ev.val.offs is not None
    assert len(ev.bank) == 24 and len(ev.val) == 12
    from simclr_pytorch_distributed_amd.utils.tb import read_events
    path = eng.logger.path
    eng.run()
    events = read_events(path)
    losses = [v for _, t, v in events if t == "loss"]
    assert losses and all(math.isfinite(v) for v in losses)
    acc1 = [(s, v) for s, t, v in events if t == "knn/val_acc1"]
    acc5 = [(s, v) for s, t, v in events if t == "knn/val_acc5"]
    assert [s for s, _ in acc1] == [1] and 0.0 <= acc1[0][1] <= 100.0
    assert [v for _, v in acc5] == [100.0]      # 3 classes: top-5 always hits
    assert ev.bank is eng.train
    # without --val_folder the ragged store still refuses
    opt.val_folder = None
    with pytest.raises(ValueError, match="val_folder"):
        eng._build_knn(type("D", (), {"ragged": True})())
