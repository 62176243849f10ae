"""GPU: the evaluation transform kernel (csrc/kernels/aug.hip eval_crop_kernel: Resize on the
shorter side, antialiased bilinear, CenterCrop, normalize) against the independent fp64 oracle of
tests/evalcrop_oracle.py.

Acceptance for every pixel of every case, channel c:

    |out - oracle| <= 2^-8 * |oracle| + 4 * EPS_CROP_REF / std_c

2^-8 * |oracle| is the bf16 round-to-nearest bound of the stored value; EPS_CROP_REF is the
measured worst error of the fp32 CPU reference against the same oracle in colour units (the factor
4 covers fma contraction, the other summation order and the division ulps). The floor comes from
the reference, never from the kernel. The transform has no draws, so no view is excluded. The
conditions the cases rely on are asserted on the CPU in tests/test_evalcrop_oracle.py.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_oracle as O
import evalcrop_oracle as EO

pytestmark = pytest.mark.gpu


def _launch(gpu, run, idx=None):
    from simclr_pytorch_distributed_amd.data.augment import gpu_augment
    ragged = run["offs"] is not None
    return gpu_augment(run["data"].to(gpu), (run["idx"] if idx is None else idx).to(gpu), run["cfg"], 0,
                       offs=run["offs"].to(gpu) if ragged else None, hw=run["hw"].to(gpu) if ragged else None)


def _bits(t):
    return t.view(torch.int16).cpu()


@pytest.mark.parametrize("name", EO.CASES)
def test_kernel_matches_oracle(gpu, name):
    for k, run in enumerate(EO.get_case(name)):
        cfg, want = run["cfg"], run["norm"]
        out = _launch(gpu, run)
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (want.shape[0], cfg.size, cfg.size, 8)
        assert out.is_contiguous() and out.device.type == "cuda"
        out = out.float().cpu()
        assert torch.all(out[..., 3:] == 0), "padding channels 3..7 must be exactly 0"
        got = out[..., :3].double().numpy()
        assert np.isfinite(got).all()
        tol = 2.0 ** -8 * np.abs(want) + 4.0 * EO.EPS_CROP_REF / np.asarray(cfg.std)
        err = (np.abs(got - want) * np.asarray(cfg.std)).max()
        excess = (np.abs(got - want) - tol).reshape(want.shape[0], -1).max(1)
        print(f"{name}[{k}] R={cfg.resize} S={cfg.size}: worst |err| = {err:.3e} colour units (EPS_CROP_REF "
              f"{EO.EPS_CROP_REF:.1e}); worst |err| - tol = {excess.max():.3e}")
        bad = np.nonzero(excess > 0)[0]
        assert bad.size == 0, (name, k, bad.tolist(), excess[bad].tolist())


@pytest.mark.parametrize("name,row", [("identity", 0), ("imagenet", 2)])
def test_identity_is_bit_equal_to_the_evaluation_kernel(gpu, name, row):
    """At scale 1 the output is, bit for bit, what gpu_augment writes for AugConfig.evaluation on
    the same image cropped on the host at (top, left) and passed as a dense store: the new
    kernel's normalize and rounding are the existing kernel's."""
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, gpu_augment
    (run,) = EO.get_case(name)
    cfg = run["cfg"]
    S = cfg.size
    src = int(run["idx"][row])
    img = torch.from_numpy(O.image(run, src))
    assert EO.resized_hw(img.shape[0], img.shape[1], cfg.resize) == tuple(img.shape[:2])
    top, left = run["offsets"][row]
    crop = img[top:top + S, left:left + S].contiguous().unsqueeze(0)
    want = gpu_augment(crop.to(gpu), torch.zeros(1, dtype=torch.long, device=gpu),
                       AugConfig.evaluation(S, cfg.mean, cfg.std), 0)
    got = _launch(gpu, run)[row:row + 1]
    assert torch.equal(_bits(got), _bits(want))


def test_pure_function_per_image(gpu):
    """An image's output does not depend on its position or neighbours in idx, and two identical
    calls are bit-equal."""
    (run,) = EO.get_case("ragged_mix")
    a = _bits(_launch(gpu, run))
    assert torch.equal(a, _bits(_launch(gpu, run)))
    single = {}
    for row, s in enumerate(int(i) for i in run["idx"]):
        if s not in single:
            single[s] = _bits(_launch(gpu, run, idx=torch.tensor([s])))[0]
        assert torch.equal(a[row], single[s]), (row, s)
    (big,) = EO.get_case("imagenet")
    assert torch.equal(_bits(_launch(gpu, big)), _bits(_launch(gpu, big)))


def test_binding_rejects_bad_requests(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    mean, std = [0.5, 0.5, 0.5], [0.2, 0.2, 0.2]
    data = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=gpu)
    idx = torch.zeros(2, dtype=torch.long, device=gpu)
    flat = torch.zeros(2 * 8 * 8 * 3, dtype=torch.uint8, device=gpu)
    offs = torch.tensor([0, 192], dtype=torch.long, device=gpu)
    hw = torch.tensor([[8, 8], [8, 8]], dtype=torch.int32, device=gpu)
    assert tuple(m.gpu_eval_crop(data, idx, 8, 8, mean, std).shape) == (2, 8, 8, 8)
    assert tuple(m.gpu_eval_crop(data, idx, 4, 9, mean, std, None, None).shape) == (2, 4, 4, 8)
    assert tuple(m.gpu_eval_crop(flat, idx, 6, 8, mean, std, offs, hw).shape) == (2, 6, 6, 8)
    for args, msg in (((data, idx, 8, 7), "resize"), ((data, idx, 8, 40000), "resize"), ((data, idx, 0, 8), "crop size"),
                      ((data, idx, -1, 8), "crop size")):
        with pytest.raises(RuntimeError, match=msg):
            m.gpu_eval_crop(*args, mean, std)
    with pytest.raises(RuntimeError, match="uint8"):
        m.gpu_eval_crop(data.float(), idx, 8, 8, mean, std)
    with pytest.raises(RuntimeError, match="int64"):
        m.gpu_eval_crop(data, idx.int(), 8, 8, mean, std)
    with pytest.raises(RuntimeError, match="GPU"):
        m.gpu_eval_crop(data.cpu(), idx, 8, 8, mean, std)
    with pytest.raises(RuntimeError, match="GPU"):
        m.gpu_eval_crop(data, idx.cpu(), 8, 8, mean, std)
    with pytest.raises(RuntimeError, match="together"):
        m.gpu_eval_crop(flat, idx, 6, 8, mean, std, offs, None)
    with pytest.raises(RuntimeError, match="int32"):
        m.gpu_eval_crop(flat, idx, 6, 8, mean, std, offs, hw.long())
    with pytest.raises(RuntimeError, match="3 values"):
        m.gpu_eval_crop(data, idx, 8, 8, mean[:2], std)
    torch.cuda.synchronize()


def test_linear_engine_native_on_an_image_folder(gpu, tmp_path):
    """End to end on the native backend: one 2-step epoch, validate() and --knn on a small
    ImageFolder; the features of the ragged validation store agree with the fp32 torch encoder on
    the CPU twin's images (rounded to bf16, the network's input format) within the bar
    tests/test_gpu_probe.py::test_folded_eval_encoder holds native features to: torch bf16
    autocast's own error on the same input x 1.5 + 1e-2."""
    MEAN_S, STD_S, make_image_folder = EO.MEAN_S, EO.STD_S, EO.make_image_folder
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.data.augment import augment_reference, nhwc8_to_nchw
    from simclr_pytorch_distributed_amd.engine.knn import KnnEvaluator
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    tr, va = make_image_folder(str(tmp_path / "data"))
    opt = parse_linear(["--dataset", "path", "--data_folder", tr, "--val_folder", va, "--mean", MEAN_S, "--std", STD_S,
                        "--size", "32", "--model", "resnet18", "--backend", "native", "--knn", "--knn_k", "5",
                        "--epochs", "1", "--max_steps", "2", "--batch_size", "8", "--num_workers", "2",
                        "--work_dir", str(tmp_path / "ws")])
    eng = LinearEngine(opt, device=gpu)
    assert eng.backend == "native" and eng.folded is not None and opt.n_cls == 3
    assert eng.aug_val.resize == 37 and eng.val.offs is not None and eng.train.offs is not None
    loss, a1, a5 = eng.train_epoch(1)
    vl, v1, v5 = eng.validate()
    k1, k5 = eng.knn_eval()
    assert all(math.isfinite(v) for v in (loss, a1, a5, vl, v1, v5, k1, k5))
    assert 0.0 <= a1 <= 100.0 and 0.0 <= v1 <= v5 <= 100.0 and 0.0 <= k1 <= k5 <= 100.0
    ev = KnnEvaluator(eng.model, "native", "bf16", eng.train, eng.val, eng.aug_val, 3, k=5)
    got = ev.extract(eng.val)
    assert tuple(got.shape) == (12, 512) and torch.isfinite(got).all()
    twin = augment_reference(eng.val.images, torch.arange(12), eng.aug_val, 0, eng.val.offs, eng.val.hw)
    x = nhwc8_to_nchw(twin).to(torch.bfloat16).float().to(gpu)
    with torch.no_grad():
        ref = F.normalize(eng.model.encoder(x).float(), dim=1)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ac = F.normalize(eng.model.encoder(x).float(), dim=1)
    e_n = float((got - ref).norm() / ref.norm())
    e_c = float((ac - ref).norm() / ref.norm())
    print(f"ragged val features: native rel error {e_n:.4g} (autocast {e_c:.4g})")
    assert e_n <= 1.5 * e_c + 1e-2


CHECKED_SCRIPT = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
from simclr_pytorch_distributed_amd.ops import _ext
assert _ext.require().__name__.endswith("_C_checked")
import evalcrop_oracle as EO
from simclr_pytorch_distributed_amd.data.augment import gpu_augment
for name in ("ragged_mix", "extreme"):
    for run in EO._BUILDERS[name]():
        gpu_augment(run["data"].cuda(), run["idx"].cuda(), run["cfg"], 0, offs=run["offs"].cuda(), hw=run["hw"].cuda())
torch.cuda.synchronize()
print("CHECKED-OK")
"""


def test_checked_build_runs_clean(gpu):
    """The tap windows and output indices under the device-side checks of the bounds-checked
    build (a violation traps the kernel and fails the subprocess)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "simclr_pytorch_distributed_amd", "_C_checked.so")), \
        "checked build not present (python csrc/build.py --checked)"
    env = dict(os.environ, SDX_CHECKED="1", SDX_AUTOBUILD="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT, os.path.join(root, "tests")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHECKED-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
