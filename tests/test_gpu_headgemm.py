"""The MFMA classifier head (csrc/kernels/head_gemm.hip, --head_gemm mfma) on the GPU: the ops
and the wrappers through the checks of headgemm_checks (every quantity within its derived bound
for the probe step, the sweep step and the CE head), run-to-run and sweep-to-single bit identity,
accumulating sinks, an untouched classifier in evaluation, the unchanged fma path behind the new
keyword, and the two engines.

Worst error / bound figures of the kernels, first run on an MI355X (printed by every test):
see the docstring of test_within_bounds.
"""
import pytest
import torch

import headgemm_checks as CK

pytestmark = pytest.mark.gpu
MOM = 0.9


class GpuImpl:
    """The interface of headgemm_checks.Twin on the extension's ops: CPU tensors in and out."""

    def __init__(self, dev, single_op=False):
        from simclr_pytorch_distributed_amd.ops import _ext
        self.m = _ext.require()
        self.dev = dev
        self.single_op = single_op      # G = 1: through linear_ce_step_mfma instead of the sweep op

    def _d(self, *ts):
        return [t.to(self.dev).contiguous() for t in ts]

    def step(self, x, W, b, labels, bufW, bufb, lrs, mom, wds, first, train):
        x, W, b, labels, bufW, bufb = self._d(x, W, b, labels, bufW, bufb)
        bw, bb = (bufW, bufb) if train else (None, None)
        if self.single_op:
            assert W.shape[0] == 1
            lg, st = self.m.linear_ce_step_mfma(x, W[0], b[0], labels, bw[0] if train else None,
                                                bb[0] if train else None, lrs[0], mom, wds[0], first, train)
            lg, st = lg[None], st[None]
        else:
            lg, st = self.m.linear_ce_sweep_step_mfma(x, W, b, labels, bw, bb, list(lrs), mom, list(wds), first, train)
        torch.cuda.synchronize()
        return dict(logits=lg.cpu(), stats=st.cpu(), W=W.cpu(), b=b.cpu(), bufW=bufW.cpu(), bufb=bufb.cpu())

    def ce(self, x, W, b, labels, gout, dW0, db0):
        x, W, b, labels, dW, db = self._d(x, W, b, labels, dW0, db0)
        go = torch.tensor(gout, dtype=torch.float32, device=self.dev)
        logits, dz, rowstat, stats, loss = self.m.ce_head_fwd_mfma(x, W, b, labels, False)
        dX = self.m.ce_head_bwd_mfma(x, dz, W, go, rowstat, stats, loss, dW, db, True)
        torch.cuda.synchronize()
        return dict(logits=logits.cpu(), dz=dz.cpu(), rowstat=rowstat.cpu(), stats=stats.cpu(), loss=loss.cpu(),
                    dX=dX.cpu(), dW=dW.cpu(), db=db.cpu())


@pytest.mark.parametrize("name", CK.case_names())
def test_within_bounds(gpu, name):
    """Probe step (G = 1 cases: the single-head op), sweep step and CE head, the first and a later
    SGD step and an evaluation, a label equal to C − 1, an out-of-range label, gout = 1.7.

    Worst error / bound over the nine cases on an MI355X: logits 0.04, row loss 0.31, dz 0.47,
    Σ loss 0.11, W 0.50, b 0.49, bufW 0.43, bufb 0.41, dX 0.04, dW 0.95, db 0.94 (dW / db are
    near 1 where the sink's own rounding u·|dW| is the whole budget: G·C = 1030 classes of B = 5
    rows; the GEMM part of the bound is used to a few per cent)."""
    c = CK.case(name)
    worst = CK.Worst()
    CK.run_steps(GpuImpl(gpu), c, worst)
    if c.G == 1:
        CK.run_steps(GpuImpl(gpu, single_op=True), c, worst)
    CK.run_ce(GpuImpl(gpu), c, worst)
    print(f"{name}: worst error/bound  {worst.report()}")


@pytest.mark.parametrize("name", ["g3_b31_c17", "b31_k2048_c1000", "g16_b5_c1030"])
def test_two_runs_are_bit_identical(gpu, name):
    c = CK.case(name)
    runs = []
    for _ in range(2):
        outs = []
        CK.run_steps(GpuImpl(gpu), c, None, collect=outs)
        outs.append(CK.run_ce(GpuImpl(gpu), c))
        runs.append(outs)
    for a, b in zip(*runs):
        for k in a:
            CK.same_bits(k, torch.nan_to_num(a[k], nan=-1.0), torch.nan_to_num(b[k], nan=-1.0), name)


@pytest.mark.parametrize("name", ["g3_b31_c17", "g3_b5_k192_c65", "g16_b5_c1030", "g3_b65_k192_c17"])
def test_sweep_head_is_the_single_head_step(gpu, name):
    """Head g of a sweep against linear_ce_step_mfma alone with its (lr, wd): 3 consecutive steps."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    c = CK.case(name)
    d = lambda t: t.to(gpu).contiguous()  # noqa: E731
    x, y = d(c.x), d(c.labels)
    W, b, bufW, bufb = d(c.W), d(c.b), d(c.bufW), d(c.bufb)
    singles = [[d(t[g]) for t in (c.W, c.b, c.bufW, c.bufb)] for g in range(c.G)]
    for step in range(3):
        lg, st = m.linear_ce_sweep_step_mfma(x, W, b, y, bufW, bufb, c.lrs, MOM, c.wds, step == 0, True)
        for g, (w1, b1, bw1, bb1) in enumerate(singles):
            lg1, st1 = m.linear_ce_step_mfma(x, w1, b1, y, bw1, bb1, c.lrs[g], MOM, c.wds[g], step == 0, True)
            ctx = f"{name} step {step} head {g}"
            for k, a, r in (("logits", lg[g], lg1), ("stats", st[g], st1), ("W", W[g], w1), ("b", b[g], b1),
                            ("bufW", bufW[g], bw1), ("bufb", bufb[g], bb1)):
                CK.same_bits(k, torch.nan_to_num(a.cpu(), nan=-1.0), torch.nan_to_num(r.cpu(), nan=-1.0), ctx)
    le, se = m.linear_ce_sweep_step_mfma(x, W, b, y, None, None, c.lrs, 0.0, c.wds, False, False)
    for g, (w1, b1, _, _) in enumerate(singles):
        l1, s1 = m.linear_ce_step_mfma(x, w1, b1, y, None, None, 0.0, 0.0, 0.0, False, False)
        CK.same_bits("eval logits", le[g].cpu(), l1.cpu(), name)
        CK.same_bits("eval stats", torch.nan_to_num(se[g].cpu(), nan=-1.0), torch.nan_to_num(s1.cpu(), nan=-1.0), name)


def test_ce_sinks_accumulate_over_two_backwards(gpu):
    """Two backwards into one sink through the autograd node: the second adds to the first
    (checked against the bounds with the first backward's result as the sink's start)."""
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce_logits, supported
    c = CK.case("b33_k192_c63")
    fc = torch.nn.Linear(c.K, c.C).to(gpu)
    assert supported(fc, "mfma") and not supported(fc)          # K = 192 is outside the fma range
    with torch.no_grad():
        fc.weight.copy_(c.W[0])
        fc.bias.copy_(c.b[0])
    fc.weight.grad = c.dW0.to(gpu).clone()
    fc.bias.grad = c.db0.to(gpu).clone()
    outs = []
    for _ in range(2):
        feat = c.x.to(gpu).requires_grad_(True)
        loss, stats, logits = classifier_ce_logits(feat, fc, c.labels.to(gpu), gemm="mfma")
        (loss * c.gout).backward()
        torch.cuda.synchronize()
        outs.append(dict(dW=fc.weight.grad.cpu().clone(), db=fc.bias.grad.cpu().clone(), dX=feat.grad.cpu().clone(),
                         loss=loss.detach().cpu(), stats=stats.cpu(), logits=logits.cpu()))
    direct = GpuImpl(gpu).ce(c.x, c.W[0], c.b[0], c.labels, c.gout, c.dW0.clone(), c.db0.clone())
    for k in ("dW", "db", "dX", "logits", "stats", "loss"):                 # the node is the two ops
        CK.same_bits(k, torch.nan_to_num(outs[0][k], nan=-1.0), torch.nan_to_num(direct[k], nan=-1.0), "first backward")
    second = GpuImpl(gpu).ce(c.x, c.W[0], c.b[0], c.labels, c.gout, outs[0]["dW"].clone(), outs[0]["db"].clone())
    CK.same_bits("dW", outs[1]["dW"], second["dW"], "second backward")
    CK.same_bits("db", outs[1]["db"], second["db"], "second backward")
    assert not torch.equal(outs[1]["dW"], outs[0]["dW"])
    # and the increment is the gradient: within the dW bound with the first result as the start
    c2 = CK.Case("b33_k192_c63", c.G, c.B, c.K, c.C, True, 100 + CK.case_names().index("b33_k192_c63"))
    c2.dW0, c2.db0 = outs[0]["dW"], outs[0]["db"]
    CK.check_ce(None, c2, second)


def test_wrappers_and_the_fma_keyword(gpu):
    """NativeLinearCE / NativeLinearSweep with gemm="mfma" are the ops; gemm="fma" through the new
    keyword is bit-identical to a call without it (probe, sweep and CE head)."""
    from simclr_pytorch_distributed_amd.models.resnet import LinearClassifier
    from simclr_pytorch_distributed_amd.ops import ce_head, linear_probe
    torch.manual_seed(3)
    B, K, C = 33, 512, 10
    x = torch.randn(B, K, device=gpu)
    y = torch.randint(0, C, (B,), device=gpu)
    base = LinearClassifier("resnet18", C).to(gpu)
    assert base.fc.in_features == K

    def probe(**kw):
        cl = LinearClassifier("resnet18", C).to(gpu)
        cl.load_state_dict(base.state_dict())
        p = linear_probe.NativeLinearCE(cl, MOM, 1e-3, **kw)
        outs = [p.train_batch(x, y, 0.1) for _ in range(2)] + [p.eval_batch(x, y)]
        return [t.cpu() for o in outs for t in o] + [cl.fc.weight.detach().cpu(), cl.fc.bias.detach().cpu()]

    def sweep(**kw):
        s = linear_probe.NativeLinearSweep(base, [0.0, 1e-3], MOM, **kw)
        outs = [s.train_batch(x, y, [0.1, 0.2]) for _ in range(2)] + [s.eval_batch(x, y)]
        return [t.cpu() for o in outs for t in o] + [s.W.cpu(), s.b.cpu()]

    def head(**kw):
        fc = torch.nn.Linear(K, C).to(gpu)
        fc.load_state_dict(base.fc.state_dict())
        f = x.clone().requires_grad_(True)
        loss, stats, logits = ce_head.classifier_ce_logits(f, fc, y, **kw)
        loss.backward()
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in (loss, stats, logits, f.grad, fc.weight.grad, fc.bias.grad)]

    for fn in (probe, sweep, head):
        plain, fma, mfma = fn(), fn(gemm="fma"), fn(gemm="mfma")
        for i, (a, b) in enumerate(zip(plain, fma)):
            CK.same_bits(f"{fn.__name__}[{i}]", a, b, "gemm='fma' keyword")
        for i, (a, b) in enumerate(zip(plain, mfma)):           # same quantities, near-fp32 agreement
            assert torch.allclose(a, b, rtol=1e-3, atol=1e-4), (fn.__name__, i)
    # the probe wrapper is the op: head 0 of the sweep wrapper, same settings, bit for bit
    p, s = probe(gemm="mfma"), sweep(gemm="mfma")
    with pytest.raises(ValueError):
        linear_probe.NativeLinearCE(base, MOM, 0.0, gemm="auto")
    assert linear_probe.supported(base, gemm="mfma") and linear_probe.sweep_supported(base, 16, gemm="mfma")
    wide = torch.nn.Module()
    wide.fc = torch.nn.Linear(192, 1030).to(gpu)
    assert linear_probe.supported(wide, gemm="mfma") and not linear_probe.supported(wide)
    for k, cc in ((96, 10), (64, 40000)):
        bad = torch.nn.Module()
        bad.fc = torch.nn.Linear(k, cc).to(gpu)
        assert not linear_probe.supported(bad, gemm="mfma")
    assert len(p) == len(s)


def test_refuses_outside_the_range_before_any_launch(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    for K, C in ((96, 10), (4160, 10), (32, 10)):
        x = torch.zeros(4, K, device=gpu)
        W = torch.full((C, K), 7.0, device=gpu)
        b = torch.full((C,), 7.0, device=gpu)
        y = torch.zeros(4, dtype=torch.long, device=gpu)
        with pytest.raises(RuntimeError):
            m.linear_ce_step_mfma(x, W, b, y, torch.zeros_like(W), torch.zeros_like(b), 0.1, MOM, 0.0, True, True)
        with pytest.raises(RuntimeError):
            m.ce_head_fwd_mfma(x, W, b, y, True)
        torch.cuda.synchronize()
        assert (W == 7.0).all() and (b == 7.0).all()
    with pytest.raises(RuntimeError):                              # 17 heads
        m.linear_ce_sweep_step_mfma(torch.zeros(4, 64, device=gpu), torch.zeros(17, 3, 64, device=gpu),
                                    torch.zeros(17, 3, device=gpu), torch.zeros(4, dtype=torch.long, device=gpu),
                                    None, None, [0.1] * 17, MOM, [0.0] * 17, False, False)


ENGINE = ["--model", "resnet18", "--backend", "native", "--synthetic", "--synthetic_size", "256", "--batch_size", "64",
          "--epochs", "2", "--max_steps", "2", "--head_gemm", "mfma"]


def test_engine_sweep_equals_single_mfma_runs(gpu, tmp_path):
    """LinearEngine --head_gemm mfma --sweep_lr 0.5 2 --sweep_wd 0 1e-3 against the four single
    --head_gemm mfma runs: every head's per-epoch figures and final weights are the single run's."""
    from simclr_pytorch_distributed_amd.config import parse_linear
    from simclr_pytorch_distributed_amd.engine.linear import LinearEngine
    from test_probe_sweep import TAGS, _record
    dev = torch.device("cuda:0")
    so = parse_linear(ENGINE + ["--sweep_lr", "0.5", "2", "--sweep_wd", "0", "1e-3", "--work_dir", str(tmp_path / "sw")])
    se = LinearEngine(so, device=dev)
    assert se.head_gemm == "mfma" and se.native_sweep is not None and se.native_sweep.gemm == "mfma"
    srec = _record(se)
    se.run()
    assert [(r["lr"], r["wd"]) for r in se.sweep_results] == [(0.5, 0.0), (0.5, 1e-3), (2.0, 0.0), (2.0, 1e-3)]
    for g, r in enumerate(se.sweep_results):
        po = parse_linear(ENGINE + ["--learning_rate", str(r["lr"]), "--weight_decay", str(r["wd"]),
                                    "--work_dir", str(tmp_path / f"s{g}")])
        pe = LinearEngine(po, device=dev)
        assert pe.head_gemm == "mfma" and pe.native_ce is not None and pe.native_ce.gemm == "mfma"
        prec = _record(pe)
        pres = pe.run()
        for t in TAGS:
            got = [(v, s) for tag, v, s in srec if tag == f"classifier/{t}/h{g}"]
            want = [(v, s) for tag, v, s in prec if tag == f"classifier/{t}"]
            assert len(want) == 2 and got == want, (g, t, got, want)
        assert (r["best_acc"], r["best_acc5"]) == pres
        st = se.head_state(g)
        assert torch.equal(st["fc.weight"], pe.classifier.fc.weight) and torch.equal(st["fc.bias"], pe.classifier.fc.bias)


def test_supervised_step_puts_the_head_gradients_in_the_flat_buffer(gpu, tmp_path):
    """A supervised-engine step with --head_gemm mfma: fc's gradients (views of the flat buffer)
    are those of a direct call of the node on the step's own features."""
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.data.augment import AugConfig
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    from simclr_pytorch_distributed_amd.ops import ce_head
    opt = parse_ce(["--model", "resnet18", "--synthetic", "--synthetic_size", "64", "--batch_size", "16",
                    "--learning_rate", "0.05", "--backend", "native", "--head_gemm", "mfma", "--work_dir", str(tmp_path)])
    eng = SupervisedEngine(opt, device=gpu)
    eng.model.train()
    eng.aug = AugConfig.evaluation(32, opt.mean_t, opt.std_t)
    seen = {}
    inner = ce_head.classifier_ce_logits

    def spy(feat, fc, labels, native=True, gemm="fma"):
        seen["gemm"], seen["feat"], seen["labels"] = gemm, feat.detach().clone(), labels.clone()
        seen["W"], seen["b"] = fc.weight.detach().clone(), fc.bias.detach().clone()
        return inner(feat, fc, labels, native, gemm)

    ce_head.classifier_ce_logits = spy
    try:
        idx = torch.arange(16, device=gpu)
        st = eng.train_step(idx, eng.train.labels[idx], 1, 0, 1)
    finally:
        ce_head.classifier_ce_logits = inner
    torch.cuda.synchronize()
    assert eng.head_gemm() == "mfma" and seen["gemm"] == "mfma"
    fc = eng.model.fc
    assert fc.weight.grad is not None and fc.weight.grad.data_ptr() != 0
    m = eng.runner  # noqa: F841  (the engine owns the flat buffer the gradients are views of)
    x = seen["feat"].float().contiguous()
    from simclr_pytorch_distributed_amd.ops import _ext
    ext = _ext.require()
    logits, dz, rowstat, stats, loss = ext.ce_head_fwd_mfma(x, seen["W"], seen["b"], seen["labels"].long(), False)
    dW, db = torch.zeros_like(seen["W"]), torch.zeros_like(seen["b"])
    ext.ce_head_bwd_mfma(x, dz, seen["W"], torch.ones((), device=gpu), rowstat, stats, loss, dW, db, True)
    torch.cuda.synchronize()
    CK.same_bits("loss", st["loss_local"].reshape(1).cpu(), loss.reshape(1).cpu(), "engine step")
    CK.same_bits("stats", st["stats"].cpu(), stats.cpu(), "engine step")
    CK.same_bits("fc.weight.grad", fc.weight.grad.cpu(), dW.cpu(), "engine step")
    CK.same_bits("fc.bias.grad", fc.bias.grad.cpu(), db.cpu(), "engine step")
