"""GPU: the augmentation kernel with the Gaussian-blur stage (csrc/kernels/aug.hip
aug_blur_kernel) against the independent fp64 oracle of tests/blur_oracle.py.

Acceptance for every view that is not fragile (aug_oracle.redraw_crop), every pixel, channel c:

    |out - oracle| <= 2^-8 * |oracle| + 4 * eps_ref(case) / std_c

2^-8 * |oracle| is the bf16 round-to-nearest bound of the stored value; eps_ref is the measured
worst error of the fp32 CPU reference against the same oracle in colour units (the factor 4
covers fma contraction and the GPU's expf and division ulps): EPS_BLUR_REF for blur_224_k23,
which sets it, and the sharper EPS_BLUR_REF_REST, measured over the other cases, for those. The
floor comes from the reference, never from the kernel. The conditions a case relies on (blur
outcome shares, fragile share, r = S - 1, the automatic kernel sizes, LDS above 64 KiB, more
than one column strip with a partial last one) are asserted on the CPU in
tests/test_blur_oracle.py::test_case_conditions.
"""
import numpy as np
import pytest
import torch

import blur_oracle as BO

pytestmark = pytest.mark.gpu


def _run(gpu, case, seed=None, seed_t=None):
    from simclr_pytorch_distributed_amd.data.augment import gpu_augment
    ragged = case["offs"] is not None
    return gpu_augment(case["data"].to(gpu), case["idx"].to(gpu), case["cfg"], case["seed"] if seed is None else seed,
                       seed_t=seed_t, offs=case["offs"].to(gpu) if ragged else None,
                       hw=case["hw"].to(gpu) if ragged else None)


@pytest.mark.parametrize("name", BO.CASES)
def test_kernel_matches_oracle(gpu, name):
    case = BO.get_case(name)
    cfg, want = case["cfg"], case["norm"]
    out = _run(gpu, case)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (want.shape[0], cfg.size, cfg.size, 8)
    assert out.is_contiguous() and out.device.type == "cuda"
    out = out.float().cpu()
    assert torch.all(out[..., 3:] == 0), "padding channels 3..7 must be exactly 0"
    got = out[..., :3].double().numpy()
    tol = 2.0 ** -8 * np.abs(want) + 4.0 * BO.eps_ref(name) / np.asarray(cfg.std)
    excess = (np.abs(got - want) - tol).reshape(want.shape[0], -1).max(1)
    keep = np.array([not r["fragile"] for r in case["rows"]])
    err = (np.abs(got - want) * np.asarray(cfg.std)).reshape(want.shape[0], -1).max(1)
    print(f"{name}: {int((~keep).sum())} fragile of {len(keep)}; worst |err| = {err[keep].max():.3e} colour units "
          f"(floor of the case {BO.eps_ref(name):.1e}); worst |err| - tol = {excess[keep].max():.3e}")
    bad = np.nonzero(keep & (excess > 0))[0]
    assert bad.size == 0, (name, bad.tolist(), excess[bad].tolist())


def test_unblurred_views_are_bit_equal_to_the_blur_off_kernel(gpu):
    """blur_simclr_32: a view whose blur draw is false is exactly what gpu_augment writes for
    the same seed with the stage off; a view whose draw is true is not."""
    case = BO.get_case("blur_simclr_32")
    on = _run(gpu, case).view(torch.int16).cpu()
    off = _run(gpu, BO.without_blur(case)).view(torch.int16).cpu()
    assert on.shape == off.shape
    for i, r in enumerate(case["rows"]):
        assert torch.equal(on[i], off[i]) == (not r["p"]["blur"]), (i, r["p"]["blur"], r["p"]["sigma"])


def test_rows_per_round_do_not_change_the_output(gpu):
    """Rows per barrier round only schedule the stream through LDS: every setting computes each
    pixel with the same arithmetic in the same order."""
    from simclr_pytorch_distributed_amd.data.augment import gpu_augment
    # blur_strips: several rows per round in column strips (its automatic plan takes one row)
    for name, all_rows in (("blur_odd_row", (1, 3, 16)), ("blur_simclr_32", (1, 3, 16)), ("blur_strips", (3,))):
        case = BO.get_case(name)
        ragged = case["offs"] is not None
        kw = dict(offs=case["offs"].to(gpu), hw=case["hw"].to(gpu)) if ragged else {}
        data, idx = case["data"].to(gpu), case["idx"].to(gpu)
        auto = gpu_augment(data, idx, case["cfg"], case["seed"], **kw).view(torch.int16)
        for rows in all_rows:
            got = gpu_augment(data, idx, case["cfg"], case["seed"], _blur_rows=rows, **kw).view(torch.int16)
            assert torch.equal(got, auto), (name, rows)


def test_seed_tensor_and_repeatability(gpu):
    """The device-resident seed overrides the host one, and a call is a pure function of
    (data, idx, cfg, seed): bit-equal outputs."""
    case = BO.get_case("blur_simclr_32")
    a = _run(gpu, case, seed=77)
    b = _run(gpu, case, seed=77)
    c = _run(gpu, case, seed=1, seed_t=torch.tensor([77], dtype=torch.int64, device=gpu))
    d = _run(gpu, case, seed=78)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    assert not torch.equal(a.view(torch.int16), d.view(torch.int16))
    big = BO.get_case("blur_224_k23")
    assert torch.equal(_run(gpu, big).view(torch.int16), _run(gpu, big).view(torch.int16))


def test_binding_rejects_bad_requests(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    mean, std = [0.5, 0.5, 0.5], [0.2, 0.2, 0.2]

    def call(data, idx, S=8, k=3, lo=0.1, hi=2.0, p=0.5, rows=0):
        return m.gpu_augment_blur(data, idx, S, 2, 0, mean, std, 0.2, 1.0, 0.75, 4 / 3, 0.8, 0.4, 0.4, 0.4, 0.1, 0.2,
                                  True, True, p, k, lo, hi, None, None, None, rows)

    data = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=gpu)
    idx = torch.zeros(2, dtype=torch.long, device=gpu)
    assert tuple(call(data, idx).shape) == (4, 8, 8, 8)
    assert tuple(call(data, idx, k=0).shape) == (4, 8, 8, 8)           # automatic size
    assert tuple(call(data, idx, k=15).shape) == (4, 8, 8, 8)          # r = S - 1
    for kw, msg in ((dict(k=4), "odd"), (dict(k=1), "odd"), (dict(k=17), "radius"), (dict(lo=0.0), "sigma"),
                    (dict(lo=2.0, hi=1.0), "sigma"), (dict(p=1.5), "blur_p"), (dict(rows=17), "rows"),
                    (dict(S=256, k=255), "LDS")):
        with pytest.raises(RuntimeError, match=msg):
            call(data, idx, **kw)
    with pytest.raises(RuntimeError, match="uint8"):
        call(data.float(), idx)
    with pytest.raises(RuntimeError, match="int64"):
        call(data, idx.int())
    with pytest.raises(RuntimeError, match="GPU"):
        call(data.cpu(), idx)
    with pytest.raises(RuntimeError, match="GPU"):
        call(data, idx.cpu())
    torch.cuda.synchronize()


def test_cuda_graph_replays_draw_fresh_blurred_views(gpu, tmp_path):
    """--cuda_graph with --blur_p at 224 (LDS above 64 KiB, so the launcher raises the kernel's
    dynamic-LDS limit; the capture's warm-up steps have done that before the capture starts):
    the views of every replay are, bit for bit, what an eager launch writes for that step's seed,
    they differ from step to step, and the blur stage ran."""
    import dataclasses
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.data.augment import gpu_augment
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    opt = parse_pretrain(["--batch_size", "8", "--synthetic", "--synthetic_size", "16", "--work_dir", str(tmp_path),
                          "--model", "resnet50", "--backend", "native", "--stem", "imagenet", "--size", "224",
                          "--learning_rate", "0.05", "--blur_p", "0.5", "--cuda_graph"], make_dirs=False)
    eng = PretrainEngine(opt)
    assert eng.backend == "native" and eng.aug.blur_p == 0.5 and eng.aug.blur_k == 23
    seen = []
    make_views = eng.make_views

    def recording(*a, **kw):     # holds the captured step's view tensor, so the graph's pool keeps it
        seen.append(make_views(*a, **kw))
        return seen[-1]

    eng.make_views = recording
    idx = torch.arange(8, device=gpu)
    assert eng.enable_cuda_graph(idx)
    static = seen[-1]
    n_calls = len(seen)
    views = []
    for it in range(2):
        eng.train_step(idx, 1, it, 10)
        torch.cuda.synchronize()
        assert len(seen) == n_calls, "the step was not replayed from the graph"
        views.append(static.clone())
        eager = gpu_augment(eng.train.images, idx, eng.aug, eng._seed_host, offs=eng.train.offs, hw=eng.train.hw)
        assert torch.equal(views[-1].view(torch.int16), eager.view(torch.int16)), it
        plain = gpu_augment(eng.train.images, idx, dataclasses.replace(eng.aug, blur_p=0.0), eng._seed_host,
                            offs=eng.train.offs, hw=eng.train.hw)
        same = [torch.equal(eager[i].view(torch.int16), plain[i].view(torch.int16)) for i in range(16)]
        assert 0 < sum(same) < 16, (it, same)      # blurred and un-blurred views in the batch
    assert not torch.equal(views[0].view(torch.int16), views[1].view(torch.int16))


CHECKED_SCRIPT = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
from simclr_pytorch_distributed_amd.ops import _ext
assert _ext.require().__name__.endswith("_C_checked")
import blur_oracle as BO
from simclr_pytorch_distributed_amd.data.augment import gpu_augment
for name in ("blur_reflect_max", "blur_odd_row", "blur_ragged", "blur_224_k23", "blur_strips"):
    case = BO._BUILDERS[name]()
    ragged = case["offs"] is not None
    for rows in (0, 1, 3):
        gpu_augment(case["data"].cuda(), case["idx"].cuda(), case["cfg"], case["seed"],
                    offs=case["offs"].cuda() if ragged else None, hw=case["hw"].cuda() if ragged else None,
                    _blur_rows=rows)
torch.cuda.synchronize()
print("CHECKED-OK")
"""


def test_checked_build_runs_clean(gpu):
    """The ring, staging-row and output indices under the device-side checks of the
    bounds-checked build (a violation traps the kernel and fails the subprocess)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "simclr_pytorch_distributed_amd", "_C_checked.so")), \
        "checked build not present (python csrc/build.py --checked)"
    env = dict(os.environ, SDX_CHECKED="1", SDX_AUTOBUILD="0", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT, os.path.join(root, "tests")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHECKED-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
