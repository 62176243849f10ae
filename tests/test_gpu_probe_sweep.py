"""The linear-probe sweep kernels (csrc/kernels/linear_ce_sweep.hip, op linear_ce_sweep_step,
ops/linear_probe.py NativeLinearSweep): head g of a sweep step is BIT-identical to the
single-head kernels (linear_ce_step, NativeLinearCE) run alone with that head's learning rate and
weight decay; heads are independent; nothing outside the parameter views is written; everything
outside the supported set is refused before a launch; and LinearEngine with --sweep_lr reports,
per head, exactly what a single run with that learning rate reports."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MOM = 0.9


def _init(G, K, C, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    W0 = (torch.randn(C, K, generator=g) * 0.05).to(gpu)
    b0 = (torch.randn(C, generator=g) * 0.1).to(gpu)
    return W0, b0


def _batch(B, K, C, gpu, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, generator=g).relu().to(gpu)
    y = torch.randint(0, C, (B,), generator=g).to(gpu)
    return x, y


def _stack(t, G):
    return t.unsqueeze(0).repeat(G, *([1] * t.dim())).contiguous()


# per case: (G, B, K, C, base lrs, wds); the step lrs are the base lrs times a per-step factor
CASES = [
    (1, 5, 64, 3, [30.0], [1e-3]),                                   # idle waves, a partial 4-row block
    (3, 1, 64, 1, [0.01, 1.0, 30.0], [0.0, 1e-3, 0.0]),
    (2, 37, 512, 10, [30.0, 0.01], [1e-3, 0.0]),                     # C % 4 != 0
    (3, 37, 2048, 70, [0.01, 30.0, 0.01], [0.0, 1e-3, 0.0]),         # lane-strided softmax loop, KJ = 32;
                                                                    # heads 0 and 2 have identical settings
    (16, 6, 512, 10, [0.01 * (30.0 / 0.01) ** (i / 15.0) for i in range(16)],
     [0.0 if i % 2 else 1e-3 for i in range(16)]),                   # the head cap
    (2, 6, 2048, 1000, [0.01, 30.0], [1e-3, 0.0]),                   # G·C > 1024: the LDS tile reused per head
]
STEP_FACTORS = [1.0, 0.5, 0.1]
ONE_HEAD_FACTORS = [1.0, 0.1, 1.0 / 3000.0]        # a single head spans 30 ... 0.01 over its steps


@pytest.mark.parametrize("G,B,K,C,lrs,wds", CASES, ids=[f"G{c[0]}-B{c[1]}-K{c[2]}-C{c[3]}" for c in CASES])
def test_heads_bit_identical_to_single_head_kernels(gpu, G, B, K, C, lrs, wds):
    from simclr_pytorch_distributed_amd.ops import _ext
    from simclr_pytorch_distributed_amd.ops.linear_probe import NativeLinearCE
    m = _ext.require()
    assert len(lrs) == len(wds) == G
    assert G == 1 or (min(lrs) <= 0.01 and max(lrs) >= 30.0 and 0.0 in wds and 1e-3 in wds)
    W0, b0 = _init(G, K, C, gpu, 17 * G + C)
    W, b = _stack(W0, G), _stack(b0, G)
    bufW, bufb = torch.zeros_like(W), torch.zeros_like(b)
    singles = []
    for g in range(G):
        fc = torch.nn.Linear(K, C).to(gpu)
        with torch.no_grad():
            fc.weight.copy_(W0)
            fc.bias.copy_(b0)
        holder = torch.nn.Module()
        holder.fc = fc
        singles.append(NativeLinearCE(holder, MOM, wds[g]))

    def compare(out, st, ref, what):
        for g in range(G):
            lo, so = ref[g]
            assert torch.equal(out[g], lo), (what, "logits", g)
            assert torch.equal(st[g], so), (what, "stats", g)
            assert torch.equal(W[g], singles[g].W.data) and torch.equal(b[g], singles[g].b.data), (what, "W/b", g)
            assert torch.equal(bufW[g], singles[g].bufW) and torch.equal(bufb[g], singles[g].bufb), (what, "buf", g)

    for step, f in enumerate(STEP_FACTORS if G > 1 else ONE_HEAD_FACTORS):
        x, y = _batch(B, K, C, gpu, 100 + step)
        step_lrs = [lr * f for lr in lrs]
        out, st = m.linear_ce_sweep_step(x, W, b, y, bufW, bufb, step_lrs, MOM, wds, step == 0, True)
        ref = [singles[g].train_batch(x, y, step_lrs[g]) for g in range(G)]
        torch.cuda.synchronize()
        assert out.shape == (G, B, C) and st.shape == (G, 3)
        assert torch.isfinite(out).all() and torch.isfinite(W).all()
        compare(out, st, ref, f"step {step}")
    x, y = _batch(B, K, C, gpu, 200)
    keep = (W.clone(), b.clone(), bufW.clone(), bufb.clone())
    out, st = m.linear_ce_sweep_step(x, W, b, y, None, None, [0.0] * G, 0.0, [0.0] * G, False, False)
    ref = [singles[g].eval_batch(x, y) for g in range(G)]
    torch.cuda.synchronize()
    compare(out, st, ref, "eval")
    for t, k in zip((W, b, bufW, bufb), keep):
        assert torch.equal(t, k)                                     # an evaluation call writes no parameter
    if (G, K, C) == (3, 2048, 70):
        # two heads with identical settings are bit-equal to each other, and differ from the third
        for t in (W, b, bufW, bufb, out, st):
            assert torch.equal(t[0], t[2])
        assert not torch.equal(W[0], W[1])


def test_native_sweep_class_matches_native_linear_ce(gpu):
    """NativeLinearSweep: every head starts from the classifier's weights; head_state loads."""
    from simclr_pytorch_distributed_amd.models.resnet import LinearClassifier
    from simclr_pytorch_distributed_amd.ops.linear_probe import NativeLinearCE, NativeLinearSweep, sweep_supported
    torch.manual_seed(3)
    clf = LinearClassifier("resnet18", 10).to(gpu)
    assert sweep_supported(clf, 3) and sweep_supported(clf, 16)
    assert not sweep_supported(clf, 0) and not sweep_supported(clf, 17)
    assert not sweep_supported(LinearClassifier("resnet18", 10), 3)          # a CPU classifier
    wds, lrs = [0.0, 1e-3, 0.0], [0.5, 1.0, 2.0]
    sw = NativeLinearSweep(clf, wds, MOM)
    singles = []
    for g in range(3):
        c = LinearClassifier("resnet18", 10).to(gpu)
        c.load_state_dict(clf.state_dict())
        singles.append((c, NativeLinearCE(c, MOM, wds[g])))
    for step in range(2):
        x, y = _batch(20, 512, 10, gpu, 300 + step)
        out, st = sw.train_batch(x, y, lrs)
        for g, (c, ce) in enumerate(singles):
            lo, so = ce.train_batch(x, y, lrs[g])
            assert torch.equal(out[g], lo) and torch.equal(st[g], so)
    out, st = sw.eval_batch(x, y)
    for g, (c, ce) in enumerate(singles):
        lo, so = ce.eval_batch(x, y)
        assert torch.equal(out[g], lo) and torch.equal(st[g], so)
        fresh = LinearClassifier("resnet18", 10)
        fresh.load_state_dict(sw.head_state(g))
        assert torch.equal(fresh.fc.weight, c.fc.weight.cpu()) and torch.equal(fresh.fc.bias, c.fc.bias.cpu())
    with pytest.raises(ValueError):
        NativeLinearSweep(clf, [0.0] * 17, MOM)


def test_heads_are_independent(gpu):
    """Perturbing head 1's initial weights leaves every output of heads 0 and 2 bit-equal."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    G, B, K, C = 3, 9, 256, 12
    lrs, wds = [0.5, 5.0, 0.05], [1e-3, 0.0, 1e-3]
    W0, b0 = _init(G, K, C, gpu, 5)
    runs = []
    for perturb in (False, True):
        W, b = _stack(W0, G), _stack(b0, G)
        if perturb:
            W[1] += 0.25
            b[1] -= 0.5
        bufW, bufb = torch.zeros_like(W), torch.zeros_like(b)
        outs = []
        for step in range(2):
            x, y = _batch(B, K, C, gpu, 400 + step)
            out, st = m.linear_ce_sweep_step(x, W, b, y, bufW, bufb, lrs, MOM, wds, step == 0, True)
            outs += [out, st]
        runs.append(outs + [W, b, bufW, bufb])
    torch.cuda.synchronize()
    for a, p in zip(*runs):
        assert torch.equal(a[0], p[0]) and torch.equal(a[2], p[2])
        assert not torch.equal(a[1], p[1])


def _views(G, C, K, gpu, offset=4):
    """W, b, bufW, bufb as views inside larger tensors filled with 7.0 (offset in floats: 4 = 16 bytes)."""
    bigs, views = [], []
    for n, shape in ((G * C * K, (G, C, K)), (G * C, (G, C)), (G * C * K, (G, C, K)), (G * C, (G, C))):
        big = torch.full((n + 2 * offset + 8,), 7.0, device=gpu)
        bigs.append(big)
        views.append(big[offset:offset + n].view(shape))
    return bigs, views


def test_nothing_outside_the_views_is_written(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    G, B, K, C, off = 3, 7, 128, 10, 4
    bigs, (W, b, bufW, bufb) = _views(G, C, K, gpu, off)
    W0, b0 = _init(G, K, C, gpu, 6)
    W.copy_(_stack(W0, G))
    b.copy_(_stack(b0, G))
    bufW.zero_()
    bufb.zero_()
    x, y = _batch(B, K, C, gpu, 500)
    for step in range(2):
        m.linear_ce_sweep_step(x, W, b, y, bufW, bufb, [0.5, 1.0, 2.0], MOM, [0.0, 1e-3, 0.0], step == 0, True)
    torch.cuda.synchronize()
    for big, v in zip(bigs, (W, b, bufW, bufb)):
        n = v.numel()
        assert (big[:off] == 7.0).all() and (big[off + n:] == 7.0).all()
        assert not (v == 7.0).any() and torch.isfinite(v).all()
    assert not torch.equal(W[0], W0)


def _refusal_args(gpu, G=2, B=4, K=64, C=5, n_lr=None, n_wd=None):
    x = torch.full((B, K), 0.5, device=gpu)
    y = torch.zeros(B, dtype=torch.long, device=gpu)
    dst = [torch.full((G, C, K), 7.0, device=gpu), torch.full((G, C), 7.0, device=gpu),
           torch.full((G, C, K), 7.0, device=gpu), torch.full((G, C), 7.0, device=gpu)]
    lrs = [1.0] * (G if n_lr is None else n_lr)
    wds = [0.0] * (G if n_wd is None else n_wd)
    return x, y, dst, lrs, wds


@pytest.mark.parametrize("kw", [dict(G=0), dict(G=17), dict(K=96), dict(K=4096), dict(C=1025),
                                dict(n_lr=3), dict(n_wd=1)],
                         ids=["G0", "G17", "K96", "K4096", "C1025", "lrs-length", "wds-length"])
def test_refuses_unsupported_shapes(gpu, kw):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    x, y, dst, lrs, wds = _refusal_args(gpu, **kw)
    with pytest.raises(RuntimeError):
        m.linear_ce_sweep_step(x, dst[0], dst[1], y, dst[2], dst[3], lrs, MOM, wds, True, True)
    with pytest.raises(RuntimeError):
        m.linear_ce_sweep_step(x, dst[0], dst[1], y, None, None, lrs, 0.0, wds, False, False)
    torch.cuda.synchronize()
    for t in dst:
        assert (t == 7.0).all()


def test_refuses_non_contiguous_and_misaligned(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    G, B, K, C = 2, 4, 64, 5
    x, y, dst, lrs, wds = _refusal_args(gpu, G, B, K, C)
    wide = torch.full((G, C, 2 * K), 7.0, device=gpu)
    with pytest.raises(RuntimeError):                                # a non-contiguous W
        m.linear_ce_sweep_step(x, wide[:, :, :K], dst[1], y, dst[2], dst[3], lrs, MOM, wds, True, True)
    bigs, (Wm, bm, bufWm, bufbm) = _views(G, C, K, gpu, offset=1)    # 4 bytes off a 16-byte boundary
    assert Wm.is_contiguous() and Wm.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError):                                # a misaligned momentum-buffer view
        m.linear_ce_sweep_step(x, dst[0], dst[1], y, bufWm, dst[3], lrs, MOM, wds, True, True)
    with pytest.raises(RuntimeError):                                # a misaligned W view
        m.linear_ce_sweep_step(x, Wm, dst[1], y, dst[2], dst[3], lrs, MOM, wds, True, True)
    with pytest.raises(RuntimeError):                                # a training step without buffers
        m.linear_ce_sweep_step(x, dst[0], dst[1], y, None, None, lrs, MOM, wds, True, True)
    torch.cuda.synchronize()
    for t in dst + bigs + [wide]:
        assert (t == 7.0).all()


ENGINE = ["--model", "resnet18", "--backend", "native", "--synthetic", "--synthetic_size", "512", "--batch_size", "64",
          "--epochs", "2", "--max_steps", "3"]


@pytest.mark.parametrize("extra", [[], ["--cosine", "--warm"]], ids=["multistep", "cosine-warm"])
def test_engine_sweep_equals_single_runs(gpu, tmp_path, caplog, extra):
    """LinearEngine --sweep_lr 0.5 1 2 against three single runs with the same seed: every head's
    per-epoch train and validation loss / acc1 / acc5 are the single run's exactly."""
    from test_probe_sweep import check_sweep_equals_singles, run_sweep_and_singles
    lrs = [0.5, 1.0, 2.0]
    with caplog.at_level("INFO"):
        se, sres, srec, singles = run_sweep_and_singles(tmp_path, torch.device("cuda:0"), ENGINE, lrs, extra=extra)
    assert se.native_sweep is not None and se.folded is not None
    assert all(pe.native_ce is not None for _, _, pe in singles)
    check_sweep_equals_singles(se, sres, srec, singles, lrs, 2)
    for g, (_, _, pe) in enumerate(singles):
        st = se.head_state(g)
        assert torch.equal(st["fc.weight"], pe.classifier.fc.weight) and torch.equal(st["fc.bias"], pe.classifier.fc.bias)
    if extra:
        assert len({o.warmup_to for o in se.head_opts}) == 3         # the warm-up target is per head
    lines = [r.getMessage() for r in caplog.records]
    assert "best accuracy: {:.2f}, accuracy5: {:.2f}".format(*sres) in lines
    for g, r in enumerate(se.sweep_results):
        assert "head {} lr {:g} wd 0: best accuracy {:.2f}, accuracy5 {:.2f}".format(
            g, r["lr"], r["best_acc"], r["best_acc5"]) in lines
