"""GPU: augmentation kernel vs the torch reference with identical draws; fused SGD/LARS
kernels vs the torch fallback; native end-to-end step (engine) runs and is finite.

The independent checks of these two kernels live elsewhere: tests/test_gpu_augment.py (each
augmentation stage against the fp64 oracle tests/aug_oracle.py) and tests/test_gpu_optim.py
(sgd_step / lars_step on hand-made flat buffers against fp64 oracles)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_gpu_augment_matches_reference(gpu):
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, augment_reference, gpu_augment
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (40, 32, 32, 3), generator=g, dtype=torch.uint8)
    idx = torch.tensor([3, 17, 0, 39, 8, 21, 5, 11])
    for cfg in (AugConfig.simclr(32, (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)),
                AugConfig.linear_train(32, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)),
                AugConfig.evaluation(32, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))):
        out = gpu_augment(data.to(gpu), idx.to(gpu), cfg, 77).float().cpu()
        ref = augment_reference(data, idx, cfg, 77)
        assert out.shape == ref.shape
        err = (out - ref).abs().amax(dim=(1, 2, 3))
        # bf16 output; allow a rare view whose float32 crop draw rounds differently
        assert (err < 0.05).float().mean() >= 0.85, err
        assert torch.all(out[..., 3:] == 0)


def test_gpu_augment_ragged_native_resolution(gpu):
    """ImageFolder store at native resolutions (ragged: flat bytes + offsets + sizes): the
    kernel crops from each image's own pixels, same draws as the torch reference."""
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, augment_reference, gpu_augment
    g = torch.Generator().manual_seed(1)
    shapes = [(48, 64), (100, 75), (33, 33), (64, 128), (90, 40), (57, 71)]
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in shapes]
    flat = torch.cat([i.reshape(-1) for i in imgs])
    hw = torch.tensor(shapes, dtype=torch.int32)
    offs = torch.cumsum(torch.tensor([0] + [h * w * 3 for h, w in shapes[:-1]]), 0).to(torch.int64)
    idx = torch.tensor([5, 0, 3, 1, 4, 2, 3, 1])
    for cfg in (AugConfig.simclr(32, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25)),
                AugConfig.evaluation(24, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))):
        out = gpu_augment(flat.to(gpu), idx.to(gpu), cfg, 9, offs=offs.to(gpu), hw=hw.to(gpu)).float().cpu()
        ref = augment_reference(flat, idx, cfg, 9, offs, hw)
        err = (out - ref).abs().amax(dim=(1, 2, 3))
        assert (err < 0.05).float().mean() >= 0.85, err


@pytest.mark.parametrize("kind", ["sgd", "lars"])
def test_fused_optimizer_kernels(gpu, kind):
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams, FusedLARS, FusedSGD
    torch.manual_seed(0)

    def make():
        torch.manual_seed(0)
        return torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3), torch.nn.BatchNorm2d(16), torch.nn.Flatten(),
                                   torch.nn.Linear(16 * 6 * 6, 10)).to(gpu)

    a, b = make(), make()
    fa, fb = FlatParams(a), FlatParams(b)
    cls = FusedSGD if kind == "sgd" else FusedLARS
    oa = cls(fa, 0.1, 0.9, 1e-4, backend="auto")
    ob = cls(fb, 0.1, 0.9, 1e-4, backend="torch")
    assert oa.native and not ob.native
    oa.grad_scale = ob.grad_scale = 0.5
    x = torch.randn(4, 8, 8, 8, device=gpu)
    for _ in range(3):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).tanh().sum().backward()
            o.step()
    assert torch.allclose(fa.flat, fb.flat, atol=1e-5, rtol=1e-4)


def test_native_engine_step(gpu, tmp_path):
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    opt = parse_pretrain(["--batch_size", "64", "--synthetic", "--synthetic_size", "256", "--work_dir",
                          str(tmp_path), "--model", "resnet50", "--backend", "native"], make_dirs=False)
    eng = PretrainEngine(opt)
    assert eng.backend == "native"
    idx = torch.arange(64, device=gpu)
    w0 = eng.flat.flat.clone()
    st = eng.train_step(idx, 1, 0, 10)
    assert torch.isfinite(st["loss_local"]).item()
    assert not torch.equal(w0, eng.flat.flat)
    assert torch.isfinite(eng.flat.flat).all().item()


def test_early_bucket_step_matches_end_of_step(gpu, tmp_path, monkeypatch):
    """Per-bucket SGD issued as soon as each bucket's gradients are final (one rank: the bucket
    tracker without collectives, opt-in SDX_EARLY_STEP=1) == one whole-buffer SGD after backward, bit
    for bit over two steps (elementwise update, identical gradients)."""
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    args = ["--batch_size", "32", "--synthetic", "--synthetic_size", "256", "--work_dir", str(tmp_path),
            "--model", "resnet50", "--backend", "native"]
    idx = torch.arange(32, device=gpu)
    res, w0 = [], None
    for early in ("0", "1"):
        monkeypatch.setenv("SDX_EARLY_STEP", early)
        eng = PretrainEngine(parse_pretrain(args, make_dirs=False))
        assert (eng.reducer is not None) == (early == "1")
        if early == "1":
            assert len(eng.reducer.buckets) > 1 and not eng.reducer.enabled
        if w0 is None:
            w0 = eng.flat.flat.clone()
        else:
            eng.flat.flat.copy_(w0)
        for it in range(2):
            eng.train_step(idx, 1, it, 10)
        torch.cuda.synchronize()
        if early == "1":
            assert sorted(eng.reducer.launch_log[:len(eng.reducer.buckets)]) == list(range(len(eng.reducer.buckets)))
            assert eng.optimizer._applied == []
        res.append((eng.flat.flat.clone(), eng.optimizer.buf.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("kind", ["fused", "emu"])
def test_native_engine_step_emulated_syncbn(gpu, tmp_path, monkeypatch, kind):
    """The whole native training step (ResNet-50: stem, every block incl. the BN3 folds and the
    forward fold, head, loss, SGD) with SyncBN over 8 emulated ranks on this GPU
    (SDX_SYNCBN_EMU=8; 'fused': the fused xGMI exchange kernel over 8 device-memory arenas,
    'emu': reduce -> x8 -> finalize) vs the single-process step: the 8 virtual ranks hold
    identical data, so the global statistics are exact multiples of the local ones and the
    parameter update must match the single-process one."""
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    args = ["--batch_size", "64", "--synthetic", "--synthetic_size", "256", "--work_dir", str(tmp_path),
            "--model", "resnet50", "--backend", "native"]
    idx = torch.arange(64, device=gpu)
    res = []
    w0 = None
    for emu in ("0", "8"):
        monkeypatch.setenv("SDX_SYNCBN_EMU", emu)
        monkeypatch.setenv("SDX_SYNCBN_EMU_KIND", kind)
        eng = PretrainEngine(parse_pretrain(args, make_dirs=False))
        assert eng.syncbn_transport == ("none" if emu == "0" else f"emulated-8-{kind}")
        if w0 is None:
            w0 = eng.flat.flat.clone()
        else:
            eng.flat.flat.copy_(w0)
        st = eng.train_step(idx, 1, 0, 10)
        torch.cuda.synchronize()
        res.append((float(st["loss_local"]), eng.flat.flat.clone()))
    (l0, p0), (l1, p1) = res
    rel = float((p1 - p0).norm() / (p0 - w0).norm())
    print(f"emulated 8-rank SyncBN ({kind}) vs single process: loss {l1:.6f} vs {l0:.6f}, update rel {rel:.3g}")
    assert abs(l1 - l0) <= 1e-5 * abs(l0)
    assert rel < 1e-4, rel


def test_native_blocks_teacher_forced(gpu):
    """Each native block vs the torch block fed the same (bf16-rounded) input. A norm envelope
    at ResNet shapes; the strict, stage-wise check of the executor is
    tests/test_gpu_block_oracle.py."""
    from simclr_pytorch_distributed_amd.models import executor as ex
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    torch.manual_seed(0)
    m = SupConResNet("resnet50").to(gpu).to(memory_format=torch.channels_last)
    x = torch.randn(16, 3, 32, 32, device=gpu)
    with torch.no_grad():
        r = torch.relu(m.encoder.bn1(m.encoder.conv1(x)))
        for blk in m.encoder.blocks():
            xin = r.to(torch.bfloat16)
            nat = ex._bottleneck(blk, xin.permute(0, 2, 3, 1).contiguous(), True, None)
            ref = blk(xin.float())
            err = ((nat.permute(0, 3, 1, 2).float() - ref).norm() / ref.norm()).item()
            assert err < 2.5e-2, err
            r = ref


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
@pytest.mark.parametrize("variant", ["native_exec", "py_blocks", "py_prologue"])
def test_fused_blocks_match_unfused(gpu, name, variant, monkeypatch):
    """Fused block autograd (weight cache, grad sinks, fused residual-grad, with/without the
    BN+ReLU conv prologue) == per-op path. A norm envelope over the whole flat gradient; the
    strict, stage-wise check of the native executor is tests/test_gpu_block_oracle.py."""
    from simclr_pytorch_distributed_amd.ops import block, _ext
    monkeypatch.setattr(block, "FUSE_PROLOGUE", variant == "py_prologue")
    monkeypatch.setattr(block, "NATIVE_EXEC", variant == "native_exec")
    # the BN+ReLU prologue runs on the implicit-GEMM tiles: for that variant the reference side
    # does too, so both sides round alike (the tap-reuse loop sums in another order)
    m = _ext.require()
    prev = m.tap3_set(0 if variant == "py_prologue" else 1)
    try:
        _fused_vs_unfused(gpu, name, variant, monkeypatch)
    finally:
        m.tap3_set(prev)


def _fused_vs_unfused(gpu, name, variant, monkeypatch):
    from simclr_pytorch_distributed_amd.models import executor
    monkeypatch.setattr(executor, "FUSED_HEAD", False)   # same (torch) head on both sides
    from simclr_pytorch_distributed_amd.models.executor import ModelRunner, to_nhwc_input
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    torch.manual_seed(0)
    a = SupConResNet(name).to(gpu).to(memory_format=torch.channels_last)
    b = SupConResNet(name).to(gpu).to(memory_format=torch.channels_last)
    b.load_state_dict(a.state_dict())
    fa, fb = FlatParams(a), FlatParams(b)
    ra = ModelRunner(a, "native", master=fa.flat, fused=True)
    rb = ModelRunner(b, "native", master=fb.flat, fused=False)
    x = to_nhwc_input(torch.randn(16, 3, 32, 32, device=gpu))
    w = torch.randn(16, 128, device=gpu)
    for r, f in ((ra, fa), (rb, fb)):
        f.zero_grad()
        (r.forward(x) * w).sum().backward()
    torch.cuda.synchronize()   # wgrads run on the side stream
    assert torch.equal(a.encoder.layer1[0].bn1.running_mean, b.encoder.layer1[0].bn1.running_mean)
    # the fused runner counts BN passes on the host; state_dict() (checkpoints) flushes them
    assert int(a.state_dict()["encoder.bn1.num_batches_tracked"]) == 1
    assert torch.equal(a.encoder.bn1.num_batches_tracked, b.encoder.bn1.num_batches_tracked)
    ga, gb = fa.grad, fb.grad
    rel = ((ga - gb).norm() / gb.norm()).item()
    # the executor takes the block-internal BN-backward sums from the dgrad epilogue (a
    # different fp32 summation order than bn_bwd_reduce): ~1e-7 differences at the first
    # BN flip bf16 roundings that compound ~10x per block back to the stem at batch 16
    # (measured 6e-3 on resnet18; bitwise equal with SDX_DGRAD_BNSTAT=0)
    tol = 2e-2 if variant == "native_exec" else 1e-3
    assert rel < tol, rel


def test_native_engine_step_imagenet_supcon_lars(gpu, tmp_path):
    """SURVEY config 5 in miniature: SupCon, ImageNet stem (7x7/2 + max-pool) at 224x224,
    LARS, native backend — three steps: finite loss, weights move and stay finite."""
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    opt = parse_pretrain(["--batch_size", "16", "--synthetic", "--synthetic_size", "64", "--work_dir", str(tmp_path),
                          "--model", "resnet50", "--backend", "native", "--method", "SupCon", "--stem", "imagenet",
                          "--size", "224", "--optimizer", "lars", "--learning_rate", "0.3"], make_dirs=False)
    eng = PretrainEngine(opt)
    assert eng.backend == "native"
    idx = torch.arange(16, device=gpu)
    w0 = eng.flat.flat.clone()
    losses = []
    for _ in range(3):
        st = eng.train_step(idx, 1, 0, 10)
        losses.append(float(st["loss_local"].item()))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert not torch.equal(w0, eng.flat.flat)
    assert torch.isfinite(eng.flat.flat).all().item()


def test_cuda_graph_follows_eager_trajectory(gpu, tmp_path, monkeypatch):
    """--cuda_graph: the capture warm-up steps are undone, so a graphed run
    makes exactly the eager run's updates: same parameters after 3 steps on the same
    batches (up to run-to-run reduction-order noise of the split-K/atomic kernels). The
    captured chain runs its weight gradients at the eager block target here
    (SDX_GRAPH_WGRAD_BLOCKS=128): at its full-chip default they split their reductions
    differently, and at random init the rounding difference grows chaotically over steps
    (0.2 rel after 3 steps), which is not what this test checks."""
    monkeypatch.setenv("SDX_GRAPH_WGRAD_BLOCKS", "128")
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    res = []
    for graph in (False, True):
        opt = parse_pretrain(["--batch_size", "32", "--synthetic", "--synthetic_size", "128", "--work_dir",
                              str(tmp_path / f"g{int(graph)}"), "--model", "resnet18", "--backend", "native",
                              "--learning_rate", "0.05", "--seed", "3"], make_dirs=False)
        eng = PretrainEngine(opt)
        torch.manual_seed(11)
        from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
        eng.model.load_state_dict(SupConResNet("resnet18").state_dict())
        idx = torch.arange(32, device=gpu)
        if graph:
            assert eng.enable_cuda_graph(idx)
        w_init = eng.flat.flat.clone()
        for it in range(3):
            eng.train_step(idx, 1, it, 10)
        torch.cuda.synchronize()
        res.append((w_init, eng.flat.flat.clone(), eng.model.encoder.bn1.running_mean.clone()))
    (i0, w0, r0), (i1, w1, r1) = res
    assert torch.equal(i0, i1), "graph warm-up updates were not undone"
    rel = float((w0 - w1).norm() / (w0 - i0).norm())
    assert rel < 2e-2, rel
    assert torch.allclose(r0, r1, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_native_forward_backward_deterministic(gpu, name):
    """The production native path (tap-reuse and implicit-GEMM convs, per-tile BN statistics
    reduced in fp64 in tile order, deterministic split-K slabs, no atomics) is run-to-run
    bit-identical: outputs, every parameter gradient and the BN running statistics."""
    from simclr_pytorch_distributed_amd.ops import _ext
    from simclr_pytorch_distributed_amd.models.executor import ModelRunner, to_nhwc_input
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    _ext.require()
    torch.manual_seed(0)
    base = SupConResNet(name).to(gpu).to(memory_format=torch.channels_last)
    x = to_nhwc_input(torch.randn(32, 3, 32, 32, device=gpu))
    w = torch.randn(32, 128, device=gpu)

    def run():
        net = SupConResNet(name).to(gpu).to(memory_format=torch.channels_last)
        net.load_state_dict(base.state_dict())
        f = FlatParams(net)
        r = ModelRunner(net, "native", master=f.flat, fused=True)
        f.zero_grad()
        out = r.forward(x)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        bn = net.encoder.layer1[0].bn1
        return out.detach().float(), f.grad.clone(), bn.running_mean.clone(), bn.running_var.clone()

    o1, g1, rm1, rv1 = run()
    o2, g2, rm2, rv2 = run()
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2)


@pytest.mark.parametrize("shape", [(2, 112, 112, 64), (3, 15, 17, 16), (1, 8, 8, 8)])
def test_maxpool_index_backward(gpu, shape):
    """3x3/2 max-pool of the ImageNet stem: the forward's recorded first-max positions give
    exactly the recomputing backward's gradient (ties included: bf16-rounded inputs tie
    often), and both match torch's max_pool2d gradient on the same bf16 values."""
    import torch.nn.functional as F
    from simclr_pytorch_distributed_amd.ops import _ext
    from simclr_pytorch_distributed_amd.ops.pool import maxpool_nhwc
    m = _ext.require()
    N, H, W, C = shape
    g = torch.Generator(device=gpu).manual_seed(3)
    x = (torch.randn(N, H, W, C, device=gpu, generator=g) * 2).round().bfloat16()   # many exact ties
    y0 = m.maxpool_fwd(x, 3, 2, 1)
    y, idx = m.maxpool_fwd_idx(x, 3, 2, 1)
    assert torch.equal(y, y0) and idx.dtype == torch.uint8 and int(idx.max()) <= 8
    dy = torch.randn(y.shape, device=gpu, generator=g).bfloat16()
    d_old = m.maxpool_bwd(x, y, dy, 3, 2, 1)
    d_new = m.maxpool_bwd_idx(idx, dy, H, W, 3, 2, 1)
    assert torch.equal(d_old, d_new)
    xt = x.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1).backward(dy.float().permute(0, 3, 1, 2))
    assert torch.allclose(d_new.float(), xt.grad.permute(0, 2, 3, 1), atol=2e-2, rtol=1e-2)
    # autograd path (ops/pool.py) uses the index kernels
    xa = x.clone().requires_grad_(True)
    maxpool_nhwc(xa).backward(dy)
    assert torch.equal(xa.grad, d_new)


def test_weight_cache_layouts_match_torch(gpu):
    """One wprep launch (native, flat fp32 master) == the per-conv torch conversion of every
    conv / head weight into the bf16 forward [K][R][S][Cp] and dgrad [C][R][S][K] layouts,
    bit for bit (vectorised segments and the channel-padded stem)."""
    from simclr_pytorch_distributed_amd.models.executor import ModelRunner
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.optim.flat import FlatParams
    torch.manual_seed(3)
    m = SupConResNet("resnet50").to(gpu).to(memory_format=torch.channels_last)
    flat = FlatParams(m)
    with torch.no_grad():
        flat.flat.normal_()
    wc = ModelRunner(m, "native", master=flat.flat).weight_cache()
    assert wc.native
    wc.refresh()
    for cv in wc.convs:
        e = wc.entries[id(cv)]
        w = cv.weight.detach()
        w = w.view(w.shape[0], w.shape[1], 1, 1) if w.dim() == 2 else w
        krsc = w.permute(0, 2, 3, 1).to(torch.bfloat16)
        fk = wc.fwd(cv)
        assert torch.equal(fk[..., :e["C"]], krsc)
        if e["Cp"] > e["C"]:
            assert not fk[..., e["C"]:].any()
        if e["off_t"] >= 0:
            assert torch.equal(wc.dgrad(cv), krsc.permute(3, 1, 2, 0))


def test_cuda_graph_emulated_fused_syncbn(gpu, tmp_path, monkeypatch):
    """hipGraph replay of a step whose every BN runs the fused xGMI SyncBN exchange over 4
    emulated ranks (SDX_SYNCBN_EMU=4): the exchange's epoch comes from device counters, so
    each replay advances it. Graph replay follows the eager run over 5 steps (same batches):
    parameters within reduction-order noise, BN running statistics close, no flag timeout."""
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.ops import _ext
    monkeypatch.setenv("SDX_SYNCBN_EMU", "4")
    monkeypatch.setenv("SDX_SYNCBN_EMU_KIND", "fused")
    monkeypatch.setenv("SDX_GRAPH_WGRAD_BLOCKS", "128")   # the eager splits (see the test above)
    res = []
    for graph in (False, True):
        opt = parse_pretrain(["--batch_size", "32", "--synthetic", "--synthetic_size", "128", "--work_dir",
                              str(tmp_path / f"e{int(graph)}"), "--model", "resnet18", "--backend", "native",
                              "--learning_rate", "0.05", "--seed", "3"], make_dirs=False)
        eng = PretrainEngine(opt)
        assert eng.syncbn_transport == "emulated-4-fused"
        torch.manual_seed(11)
        eng.model.load_state_dict(SupConResNet("resnet18").state_dict())
        idx = torch.arange(32, device=gpu)
        if graph:
            assert eng.enable_cuda_graph(idx)
        w_init = eng.flat.flat.clone()
        losses = []
        for it in range(5):
            st = eng.train_step(idx, 1, it, 10)
            losses.append(float(st["loss_local"]))
        torch.cuda.synchronize()
        res.append((w_init, eng.flat.flat.clone(), eng.model.encoder.bn1.running_mean.clone(), losses))
    (i0, w0, r0, l0), (i1, w1, r1, l1) = res
    assert torch.equal(i0, i1)
    rel = float((w0 - w1).norm() / (w0 - i0).norm())
    assert rel < 2e-2, (rel, l0, l1)
    assert torch.allclose(r0, r1, rtol=1e-3, atol=1e-4)
    assert all(abs(a - b) < 1e-2 * max(1.0, abs(a)) for a, b in zip(l0, l1)), (l0, l1)
