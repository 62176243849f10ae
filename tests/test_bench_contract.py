"""bench.py driver contract on CPU: 2 ranks under torch.distributed.run (gloo), the torch
backend and a small model. Checks the single JSON line rank 0 prints (keys, whole-job
value, weak scaling of the global batch) — the same code path the 8-GPU scaling run takes,
minus the GPU kernels."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_json_contract(tmp_path):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "torch", "--model", "resnet18",
           "--per_gpu_batch", "4", "--full"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "host issue time (idle queue)" in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1
    assert d["scaling"] == "weak" and d["higher_is_better"] is True
    c = d["config"]
    assert c["global_batch"] == 8 and c["per_gpu_batch"] == 4 and c["parallelism"] == "dp2+syncbn"
    # the timed run is a training run: first (warm-up) and last (timed) step losses are reported
    assert isinstance(c["first_loss_local"], float) and isinstance(c["last_loss_local"], float)
    assert c["loss_steps"] == 1 + 3 + 2
    # value = whole-job images/s = global batch x steps / time
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) / d["value"] < 0.01


def _flat_total(model_name):
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    return FlatParams(SupConResNet(model_name)).total


def test_dump_outputs_sample_holds_the_indexed_positions(tmp_path):
    """``params`` / ``grads`` hold exactly the flat-buffer elements that ``sample_index`` names:
    buffers whose value at position i is i (resp. -i) come back equal to the index (resp. its
    negative); the index is strictly increasing, in range, DUMP_SAMPLE long and the same on every
    call. A buffer no longer than DUMP_SAMPLE is written whole."""
    import types

    import numpy as np
    import torch
    import bench        # the repository root is on sys.path (conftest.py)
    for total, tag in ((bench.DUMP_SAMPLE + 12345, "big"), (1000, "small")):
        pos = torch.arange(total, dtype=torch.float32)       # exact in float32 (< 2^24)
        eng = types.SimpleNamespace(flat=types.SimpleNamespace(flat=pos, grad=-pos))
        stats = {"loss_local": torch.tensor([1.5]), "note": "not a tensor"}
        for rep in ("1", "2"):
            bench._dump_outputs(str(tmp_path / (tag + rep)), eng, stats)
        d = tmp_path / (tag + "1")
        assert sorted(os.listdir(d)) == ["grads.npy", "loss_local.npy", "params.npy", "sample_index.npy"]
        idx, par, grd = (np.load(d / f) for f in ("sample_index.npy", "params.npy", "grads.npy"))
        assert idx.dtype == np.float64 and par.dtype == grd.dtype == np.float32
        assert len(idx) == min(total, bench.DUMP_SAMPLE)
        assert idx[0] >= 0 and idx[-1] < total and (np.diff(idx) > 0).all()
        np.testing.assert_array_equal(par, idx.astype(np.float32))
        np.testing.assert_array_equal(grd, -idx.astype(np.float32))
        np.testing.assert_array_equal(idx, np.load(tmp_path / (tag + "2") / "sample_index.npy"))
        if total <= bench.DUMP_SAMPLE:
            np.testing.assert_array_equal(idx, np.arange(total))
        assert float(np.load(d / "loss_local.npy")[0]) == 1.5


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain run (no --full) takes exactly warm-up + timed steps and no idle-queue diagnostic;
    --dump-outputs writes the last step's statistics and the sampled parameters / gradients as
    float32 .npy files, identical between two runs with the same arguments (seeded inputs; the
    CPU torch path is deterministic at a fixed thread count)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SDX_BENCH_CHILD")}
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    outs = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--backend", "torch", "--model", "resnet18", "--per_gpu_batch", "4", "--dump-outputs", tag]
        r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "idle queue" not in r.stderr
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert d["steps"] == 2 and d["config"]["loss_steps"] == 1 + 2 and d["ms_per_step"] > 0
        files = {f: np.load(tmp_path / tag / f) for f in sorted(os.listdir(tmp_path / tag))}
        assert {"loss_local.npy", "params.npy", "grads.npy", "sample_index.npy"} <= set(files)
        assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in files.values())
        assert files["params.npy"].shape == files["grads.npy"].shape == files["sample_index.npy"].shape
        idx = files["sample_index.npy"]
        assert (idx == np.floor(idx)).all() and idx[0] >= 0 and (np.diff(idx) > 0).all()
        assert idx[-1] < _flat_total("resnet18")
        assert abs(float(files["loss_local.npy"].reshape(-1)[0]) - d["config"]["last_loss_local"]) < 1e-3
        assert np.abs(files["grads.npy"]).max() > 0
        assert sum(v.nbytes for v in files.values()) <= 64 << 20
        outs.append(files)
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k])


def test_bench_self_launches_ranks(tmp_path):
    """``python bench.py --gpus 2`` with no external launcher starts its own 2 ranks
    (torch.distributed.run as a child process) and relays rank 0's JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SDX_BENCH_CHILD")}
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--backend", "torch", "--model", "resnet18", "--per_gpu_batch", "4"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2+syncbn"
    assert d["config"]["global_batch"] == 8


def test_bench_global_batch_is_strong_scaling(tmp_path):
    """--global_batch fixes the total batch (README headline: BS 256 over 2 GPUs)."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "1", "--warmup", "1", "--backend", "torch", "--model", "resnet18",
           "--global_batch", "8", "--dataset", "cifar100"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["scaling"] == "strong"
    assert d["config"]["global_batch"] == 8 and d["config"]["per_gpu_batch"] == 4
    assert d["config"]["dataset_shape"] == "cifar100"
