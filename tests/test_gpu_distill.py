"""The distillation forward ops (ce_head_fwd_distill, ce_head_fwd_distill_mfma: csrc/include/distill_ce.h),
the autograd node and the native engine with --distill_ckpt, against tests/distill_oracle.py under
the bounds derived in tests/distill_checks.py.

Worst error / bound seen on an MI355X: see docs/PARITY.md ("Beyond the reference").
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import distill_checks as DC
import distill_oracle as DO
import mix_checks as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m():
    from simclr_pytorch_distributed_amd.ops import _ext
    return _ext.require()


def _ops(gemm):
    m = _m()
    return (m.ce_head_fwd_distill_mfma, m.ce_head_fwd_soft_mfma, m.ce_head_fwd_mfma, m.ce_head_bwd_mfma) \
        if gemm == "mfma" else (m.ce_head_fwd_distill, m.ce_head_fwd_soft, m.ce_head_fwd, m.ce_head_bwd)


def _check_sums(ctx, rowstat, stats, loss):
    """stats = (float) of the fp64 row-order sums of the implementation's own rowstat, loss = (float)(Σ / B)."""
    sums = [0.0, 0.0, 0.0]
    for row in rowstat.double().cpu().tolist():
        sums = [s + v for s, v in zip(sums, row)]
    want = torch.tensor(sums + [sums[0] / rowstat.shape[0]], dtype=torch.float64).float().nan_to_num(-7.0)
    got = torch.cat([stats.cpu(), loss.cpu().view(1)]).nan_to_num(-7.0)
    assert torch.equal(got, want), f"{ctx}: stats / loss"


# ---- row kernels against the derived bounds -------------------------------------------------------

def _sweep(gpu, gemm, K, C, worst):
    distill, _, plain, _ = _ops(gemm)
    for B in (1, 4, 5, 37):
        x, W, b, la, lb = MC.ce_inputs(B, K, C)
        xd, Wd, bd = x.to(gpu), W.to(gpu), b.to(gpu)
        z_plain = plain(xd, Wd, bd, la.to(gpu), True)[0]
        la, lb = MC.plant_labels(z_plain.cpu(), la, lb)          # B >= 4: a −1 in either slot of the last two rows
        lad, lbd = la.to(gpu), lb.to(gpu)
        for kind in DC.TEACHERS:
            v = DC.teacher_rows(z_plain.cpu(), kind)
            vd = v.to(gpu)
            for temp in (0.5, 1.0, 4.0):
                for alpha in (0.5, 1.0):
                    for lam, eps in ((1.0, 0.0), (0.3, 0.1)):
                        ctx = f"{gemm} B={B} K={K} C={C} {kind} T={temp} alpha={alpha} lam={lam} eps={eps}"
                        logits, dz, rowstat, stats, loss = distill(xd, Wd, bd, lad, lbd, lam, eps, vd, temp, alpha, True)
                        assert torch.equal(logits, z_plain), f"{ctx}: logits differ from the plain op's"
                        DC.check_distill(worst, ctx, logits.cpu(), v, la, lb, lam, eps, temp, alpha, DO.f32(1.0 / B),
                                         rowstat.cpu(), dz.cpu())
                        _check_sums(ctx, rowstat, stats, loss)


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("C", [1, 3, 5, 65, 1000])
def test_distill_fma(gpu, K, C):
    worst = MC.Worst()
    _sweep(gpu, "fma", K, C, worst)
    print(f"distill fma K={K} C={C}: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("K", [192, 2048])
@pytest.mark.parametrize("C", [1, 3, 5, 65, 1000])
def test_distill_mfma(gpu, K, C):
    worst = MC.Worst()
    _sweep(gpu, "mfma", K, C, worst)
    print(f"distill mfma K={K} C={C}: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("gemm,K,C", [("fma", 256, 65), ("mfma", 192, 1000)])
def test_final_off_leaves_the_sums_to_the_backward_op(gpu, gemm, K, C):
    distill, _, _, bwd = _ops(gemm)
    B = 37
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    v = DC.teacher_rows(torch.zeros(B, C), "random").to(gpu)
    on = distill(x, W, b, la, lb, 0.3, 0.1, v, 4.0, 0.5, True)
    off = distill(x, W, b, la, lb, 0.3, 0.1, v, 4.0, 0.5, False)
    for name, u, w in zip(("logits", "dz", "rowstat"), on, off):
        assert torch.equal(u, w), name
    bwd(x, off[1], W, torch.ones((), device=gpu), off[2], off[3], off[4], None, None, True)
    torch.cuda.synchronize()
    assert torch.equal(on[3], off[3]) and torch.equal(on[4], off[4])
    _check_sums(f"{gemm} final", on[2], on[3], on[4])


# ---- bit equalities -------------------------------------------------------------------------------

@pytest.mark.parametrize("gemm,K,C", [("fma", 64, 5), ("fma", 256, 1000), ("mfma", 192, 65), ("mfma", 2048, 1000)])
@pytest.mark.parametrize("final", [False, True])
def test_alpha_zero_is_the_soft_op_bit_for_bit(gpu, gemm, K, C, final):
    distill, soft, _, bwd = _ops(gemm)
    for B in (1, 5, 37):
        x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
        if B >= 4:
            la[B - 1] = -1
        for kind, temp, lam, eps in (("random", 4.0, 0.3, 0.1), ("peaky", 0.5, 1.0, 0.0), ("equal", 1.0, 0.3, 0.0)):
            s = soft(x, W, b, la, lb, lam, eps, final)
            v = DC.teacher_rows(s[0].cpu(), kind).to(gpu)
            d = distill(x, W, b, la, lb, lam, eps, v, temp, 0.0, final)
            if not final:       # the backward op sums the statistics
                one = torch.ones((), device=gpu)
                for o in (s, d):
                    bwd(x, o[1], W, one, o[2], o[3], o[4], None, None, True)
            torch.cuda.synchronize()
            for name, u, w in zip(("logits", "dz", "rowstat", "stats", "loss"), s, d):
                assert torch.equal(u.view(torch.int32), w.view(torch.int32)), f"{gemm} B={B} K={K} C={C} {kind}: {name}"


@pytest.mark.parametrize("gemm,K,C", [("fma", 256, 65), ("mfma", 2048, 1000)])
def test_two_runs_are_bit_identical_and_tau_one_is_computed(gpu, gemm, K, C):
    distill, _, plain, _ = _ops(gemm)
    B = 37
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    v = DC.teacher_rows(torch.zeros(B, C), "random").to(gpu)
    r1 = distill(x, W, b, la, lb, 0.3, 0.1, v, 4.0, 0.5, True)
    r2 = distill(x, W, b, la, lb, 0.3, 0.1, v, 4.0, 0.5, True)
    for u, w in zip(r1, r2):
        assert torch.equal(u.view(torch.int32), w.view(torch.int32))
    assert torch.equal(r1[0], plain(x, W, b, la, True)[0])
    # τ = 1, teacher = student, α = 1: q_s and q_t are the same operations — kd and dz are exactly 0
    same = distill(x, W, b, la, lb, 1.0, 0.0, r1[0].clone(), 1.0, 1.0, True)
    assert float(same[1].abs().max()) == 0.0 and float(same[2][:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("gemm,K", [("fma", 64), ("mfma", 192)])
def test_unlabelled_rows(gpu, gemm, K):
    """α = 1 with label −1: finite loss, no hit. α = 0.5 with label −1: a NaN row, dz without the target."""
    distill, _, _, _ = _ops(gemm)
    B, C = 5, 10
    x, W, b, la, _ = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    un = torch.full_like(la, -1)
    v = DC.teacher_rows(torch.zeros(B, C), "random").to(gpu)
    logits, dz, rowstat, stats, loss = distill(x, W, b, un, un, 1.0, 0.0, v, 2.0, 1.0, True)
    assert bool(torch.isfinite(rowstat).all()) and bool(torch.isfinite(loss)) and float(rowstat[:, 1:].sum()) == 0.0
    DC.check_distill(MC.Worst(), "unlabelled", logits.cpu(), v.cpu(), un.cpu(), un.cpu(), 1.0, 0.0, 2.0, 1.0,
                     DO.f32(1.0 / B), rowstat.cpu(), dz.cpu())
    mixed = la.clone()
    mixed[2] = -1
    logits, dz, rowstat, stats, loss = distill(x, W, b, mixed, mixed, 1.0, 0.0, v, 2.0, 0.5, True)
    assert torch.isnan(rowstat[:, 0]).tolist() == [False, False, True, False, False]
    assert rowstat[2, 1:].tolist() == [0.0, 0.0] and bool(torch.isnan(loss)) and bool(torch.isfinite(dz).all())


# ---- the node through autograd --------------------------------------------------------------------

def _torch_distill(x, W, b, la, lb, lam, eps, v, temp, alpha, dtype):
    from simclr_pytorch_distributed_amd.ops.ce_head import soft_target
    x, W, b = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, W, b))
    z = F.linear(x, W, b)
    t = soft_target(la.cpu(), lb.cpu(), lam, eps, W.shape[0], dtype)
    kd = F.kl_div(F.log_softmax(z / temp, 1), F.softmax(v.cpu().to(dtype) / temp, 1), reduction="batchmean") * temp * temp
    loss = (1 - alpha) * F.cross_entropy(z, t) + alpha * kd
    dx, dW, db = torch.autograd.grad(loss, [x, W, b])
    return {"loss": loss.detach().double(), "dX": dx.double(), "dW": dW.double(), "db": db.double()}


def _node(gpu, gemm, x, W, b, la, lb, lam, eps, v, temp, alpha, gout):
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce_logits
    fc = torch.nn.Linear(W.shape[1], W.shape[0]).to(gpu)
    with torch.no_grad():
        fc.weight.copy_(W)
        fc.bias.copy_(b)
    xr = x.clone().requires_grad_(True)
    vr = v.clone().requires_grad_(True)
    loss, stats, logits = classifier_ce_logits(xr, fc, la, gemm=gemm, labels2=lb, lam=lam, smoothing=eps,
                                               teacher_logits=vr, temp=temp, alpha=alpha)
    assert type(loss.grad_fn).__name__.startswith("_ClassifierCE")
    loss.backward(gout)
    torch.cuda.synchronize()
    assert vr.grad is None                                   # the teacher's logits never receive a gradient
    return {"loss": loss.detach(), "stats": stats, "logits": logits, "dX": xr.grad, "dW": fc.weight.grad,
            "db": fc.bias.grad}


@pytest.mark.parametrize("B,K,C,temp,alpha", [(5, 64, 10, 2.0, 0.5), (37, 256, 1000, 4.0, 1.0)])
def test_node_through_autograd_against_fp64_torch_on_the_inputs(gpu, B, K, C, temp, alpha):
    """fma node, upstream gradient 0.5. The rule of tests/test_gpu_ce_head.py (4 x fp32 torch's own
    error + one fp32 ulp of the magnitude), extended by the derived row / dz bounds of distill_checks
    pushed through the backward's sums: |gout|·Σ_c B_dz|W|, |gout|·Σ_b B_dz|x|, |gout|·Σ_b B_dz."""
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    v = DC.teacher_rows(torch.zeros(B, C), "random").to(gpu)
    lam, eps, go = 0.3, 0.1, 0.5
    r64 = _torch_distill(x, W, b, la, lb, DO.f32(lam), DO.f32(eps), v, temp, alpha, torch.float64)
    r32 = _torch_distill(x, W, b, la, lb, DO.f32(lam), DO.f32(eps), v, temp, alpha, torch.float32)
    got = _node(gpu, "fma", x, W, b, la, lb, lam, eps, v, temp, alpha, torch.full((), go, device=gpu))
    it, tau = DO.temperature(temp)
    Bd = DC.distill_bounds(got["logits"].cpu(), v.cpu(), la.cpu(), lb.cpu(), lam, eps, it, tau, alpha, DO.f32(1.0 / B))
    bdz = Bd["dz"]
    extra = {"loss": float(Bd["row"].mean()), "dX": go * float((bdz @ W.cpu().double().abs()).max()),
             "dW": go * float((bdz.t() @ x.cpu().double().abs()).max()), "db": go * float(bdz.sum(0).max())}
    for q in ("loss", "dX", "dW", "db"):
        scale = 1.0 if q == "loss" else go
        e32 = scale * float((r32[q] - r64[q]).abs().max())
        ek = float((got[q].double().cpu() - scale * r64[q]).abs().max())
        allow = 4.0 * e32 + 2.0 ** -23 * scale * float(r64[q].abs().max()) + extra[q]
        print(f"B={B} K={K} C={C} {q}: kernel err {ek:.3e}, fp32 torch err {e32:.3e}, allowed {allow:.3e}, "
              f"ratio {ek / allow:.3f}")
        assert ek <= allow, q


@pytest.mark.parametrize("gemm,K,C", [("fma", 256, 65), ("mfma", 192, 65)])
def test_node_is_the_forward_op_and_the_unchanged_backward_op(gpu, gemm, K, C):
    distill, _, _, bwd = _ops(gemm)
    B = 37
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    v = DC.teacher_rows(torch.zeros(B, C), "peaky").to(gpu)
    go = torch.full((), 0.5, device=gpu)
    r1 = _node(gpu, gemm, x, W, b, la, lb, 0.3, 0.1, v, 0.5, 0.5, go)
    r2 = _node(gpu, gemm, x, W, b, la, lb, 0.3, 0.1, v, 0.5, 0.5, go)
    for q in r1:
        assert torch.equal(r1[q], r2[q]), q
    logits, dz, rowstat, stats, loss = distill(x, W, b, la, lb, 0.3, 0.1, v, 0.5, 0.5, False)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    dX = bwd(x, dz, W, go, rowstat, stats, loss, dW, db, True)
    torch.cuda.synchronize()
    for q, w in zip(("loss", "stats", "logits", "dX", "dW", "db"), (loss, stats, logits, dX, dW, db)):
        assert torch.equal(r1[q], w), q


# ---- refusals -------------------------------------------------------------------------------------

@pytest.mark.parametrize("gemm,K", [("fma", 64), ("mfma", 192)])
def test_refusals_leave_everything_untouched(gpu, gemm, K):
    distill, _, _, _ = _ops(gemm)
    B, C = 5, 10
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
    v = DC.teacher_rows(torch.zeros(B, C), "random").to(gpu)
    tensors = [x, W, b, la, lb, v]
    keep = [t.clone() for t in tensors]
    nan, inf = float("nan"), float("inf")
    bad = [
        dict(temp=0.0), dict(temp=-1.0), dict(temp=inf), dict(temp=nan), dict(temp=1e-45),      # τ (1e-45: 1/τ overflows)
        dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan),
        dict(lam=1.5), dict(lam=nan), dict(eps=1.0), dict(eps=-0.1),
        dict(v=v[:, :5].contiguous()), dict(v=v[:4]), dict(v=v.double()), dict(v=v.t().contiguous().t()), dict(v=v.cpu()),
        dict(lb=lb[:4]), dict(lb=lb.int()),
    ]
    base = dict(lam=0.3, eps=0.1, v=v, temp=2.0, alpha=0.5, lb=lb)
    for kw in bad:
        a = dict(base, **kw)
        with pytest.raises(RuntimeError):
            distill(x, W, b, la, a["lb"], a["lam"], a["eps"], a["v"], a["temp"], a["alpha"], True)
    if gemm == "mfma":          # the soft form's alignment rule
        xo = torch.zeros(B * K + 1, device=gpu)[1:].view(B, K)
        with pytest.raises(RuntimeError):
            distill(xo, W, b, la, lb, 0.3, 0.1, v, 2.0, 0.5, True)
    torch.cuda.synchronize()
    for t, k in zip(tensors, keep):
        assert torch.equal(t, k)
    out = distill(x, W, b, la, lb, 0.3, 0.1, v, 2.0, 0.5, True)       # and a good call still runs
    assert bool(torch.isfinite(out[4]))


# ---- native engine --------------------------------------------------------------------------------

def _teacher_ckpt(path, n_cls=10, seed=5):
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    from simclr_pytorch_distributed_amd.models.resnet import SupCEResNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        model = SupCEResNet("resnet18", n_cls)
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
        torch.save({"opt": {}, "model": ckpt_mod.model_state_with_prefix(model), "optimizer": {}, "epoch": 1}, str(path))


def _engine(tmp_path, gpu, *extra):
    from simclr_pytorch_distributed_amd.config import parse_ce
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    opt = parse_ce(["--model", "resnet18", "--synthetic", "--synthetic_size", "16", "--batch_size", "8",
                    "--learning_rate", "0.05", "--backend", "native", "--save_freq", "1", "--val_batch_size", "16",
                    "--work_dir", str(tmp_path), "--seed", "2", *extra])
    return SupervisedEngine(opt, device=gpu)


class _Spy:
    """Wraps ops of the extension module and records (arguments, result) of every call."""

    def __init__(self, monkeypatch, *names):
        self.calls = {n: [] for n in names}
        m = _m()
        for n in names:
            monkeypatch.setattr(m, n, self._wrap(n, getattr(m, n)))

    def _wrap(self, name, fn):
        def f(*a):
            r = fn(*a)
            self.calls[name].append((a, r))
            return r
        return f


def _run_steps(eng, epoch, n=2):
    eng.model.train()
    out = []
    for it, (idx, labels) in enumerate(eng.epoch_batches(epoch)):
        if it >= n:
            break
        out.append((eng.train_step(idx, labels, epoch, it, n), labels))
    torch.cuda.synchronize()
    return out


DISTILL_OPS = ("ce_head_fwd_distill", "ce_head_fwd_distill_mfma")


def test_native_engine_distils(gpu, tmp_path, monkeypatch):
    ck = tmp_path / "teacher.pth"
    _teacher_ckpt(ck)
    flags = ("--distill_ckpt", str(ck), "--distill_temp", "2", "--distill_alpha", "0.5", "--label_smoothing", "0.1")
    eng = _engine(tmp_path, gpu, *flags, "--epochs", "1")
    from simclr_pytorch_distributed_amd.ops.linear_probe import FoldedEncoder
    assert isinstance(eng._teacher_encode, FoldedEncoder) and eng._teacher_step is not None
    before = {k: t.clone() for k, t in eng.teacher.state_dict().items()}
    spy = _Spy(monkeypatch, "ce_head_fwd_distill", "ce_head_fwd_soft", "ce_head_fwd")
    steps = _run_steps(eng, 1)
    assert len(spy.calls["ce_head_fwd_distill"]) == 2 and not spy.calls["ce_head_fwd_soft"] and not spy.calls["ce_head_fwd"]
    for it, ((st, labels), (args, res)) in enumerate(zip(steps, spy.calls["ce_head_fwd_distill"])):
        assert torch.equal(args[3], labels) and args[5:7] == (1.0, 0.1) and args[8:10] == (2.0, 0.5)
        v = args[7]
        assert v.dtype == torch.float32 and tuple(v.shape) == (8, 10) and not v.requires_grad
        it_, tau = DO.temperature(2.0)
        Bd = DC.distill_bounds(res[0].cpu(), v.cpu(), args[3].cpu(), args[4].cpu(), 1.0, 0.1, it_, tau, 0.5, DO.f32(1.0 / 8))
        want = float(Bd["ref"]["loss"].mean())
        assert abs(float(st["loss_local"]) - want) <= float(Bd["row"].mean()) + MC.U * abs(want), it
    for k, t in eng.teacher.state_dict().items():
        assert torch.equal(t, before[k]), k
    # a resumed run repeats the uninterrupted one, and the checkpoint holds the student alone
    last = eng.run()
    from simclr_pytorch_distributed_amd.engine import checkpoint as ckpt_mod
    assert set(ckpt_mod.strip_prefix(ckpt_mod.load_checkpoint(last)["model"])) == set(eng.model.state_dict())
    ckpt_flat = eng.flat.flat.cpu().clone()
    spy.calls["ce_head_fwd_distill"].clear()
    straight = _run_steps(eng, 2)                        # the uninterrupted run's epoch 2
    teacher_straight = [c[0][7].clone() for c in spy.calls["ce_head_fwd_distill"]]
    spy.calls["ce_head_fwd_distill"].clear()
    eng2 = _engine(tmp_path, gpu, *flags, "--epochs", "2", "--resume", last)
    assert eng2.start_epoch == 2 and torch.equal(eng2.flat.flat.cpu(), ckpt_flat)
    resumed = _run_steps(eng2, 2)
    # the same views reach the same frozen teacher in both steps; the first step's loss is a function
    # of the restored state alone
    assert len(teacher_straight) == 2
    for u, c in zip(teacher_straight, spy.calls["ce_head_fwd_distill"]):
        assert torch.equal(u, c[0][7])
    assert torch.equal(straight[0][0]["loss_local"], resumed[0][0]["loss_local"])


def test_native_engine_alpha_one_uses_no_label(gpu, tmp_path, monkeypatch):
    ck = tmp_path / "teacher.pth"
    _teacher_ckpt(ck)
    eng = _engine(tmp_path, gpu, "--distill_ckpt", str(ck), "--label_frac", "0.1", "--head_gemm", "mfma")
    assert eng.subset.size == len(eng.train)
    spy = _Spy(monkeypatch, "ce_head_fwd_distill_mfma", "linear_ce_step_mfma")
    (st, labels), = _run_steps(eng, 1, 1)
    (args, res), = spy.calls["ce_head_fwd_distill_mfma"]
    assert len(spy.calls["linear_ce_step_mfma"]) == 1                    # the teacher's logits: the evaluation op
    assert torch.equal(args[7], spy.calls["linear_ce_step_mfma"][0][1][0]) and args[8:10] == (1.0, 1.0)
    it_, tau = DO.temperature(1.0)
    ref = DO.distill_ce(res[0].cpu(), args[7].cpu(), args[3].cpu(), args[4].cpu(), 1.0, 0.0, it_, tau, 1.0, 1.0 / 8)
    assert abs(float(st["loss_local"]) - float(ref["kd"].mean())) <= 1e-5 * max(1.0, float(ref["kd"].mean()))


def test_native_engine_flag_absent_is_todays_step(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    a = _engine(tmp_path / "a", gpu)
    assert a.teacher is None
    spy = _Spy(monkeypatch, *DISTILL_OPS)
    (sa, _), = _run_steps(a, 1, 1)
    assert not any(spy.calls.values())
    monkeypatch.setattr(SupervisedEngine, "_teacher_logits", lambda *args: pytest.fail("the teacher ran"))
    b = _engine(tmp_path / "b", gpu)

    def body(idx, labels, epoch=1, it=0):
        from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce
        zeroed, x = b._start_step(idx, epoch, it)
        loss, stats = classifier_ce(b.runner.encode(x), b.model.fc, labels, native=True, gemm=b.head_gemm())
        b._backward_and_update(loss, zeroed)
        return {"loss_local": loss.detach(), "stats": stats}

    monkeypatch.setattr(b, "_step_body", body)
    (sb, _), = _run_steps(b, 1, 1)
    assert torch.equal(sa["loss_local"], sb["loss_local"]) and torch.equal(sa["stats"], sb["stats"])
    assert torch.equal(a.flat.flat, b.flat.flat)


# ---- checked build --------------------------------------------------------------------------------

CHECKED_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from simclr_pytorch_distributed_amd.ops import _ext
m = _ext.require()
assert m.__name__.endswith("_C_checked")
import distill_checks as DC
import mix_checks as MC
for op, K in ((m.ce_head_fwd_distill, 256), (m.ce_head_fwd_distill_mfma, 192)):
    for C in (1, 65, 1000):
        a, W, b, la, lb = (t.cuda() for t in MC.ce_inputs(37, K, C))
        la[36] = -1
        v = DC.teacher_rows(torch.zeros(37, C), "peaky").cuda()
        op(a, W, b, la, lb, 0.3, 0.1, v, 0.5, 0.5, True)
        op(a, W, b, la, lb, 1.0, 0.0, v, 4.0, 1.0, False)
torch.cuda.synchronize()
print("CHECKED-OK")
"""


def test_checked_build_runs_clean(gpu):
    assert os.path.exists(os.path.join(ROOT, "simclr_pytorch_distributed_amd", "_C_checked.so")), \
        "checked build not present (python csrc/build.py --checked)"
    env = dict(os.environ, SDX_CHECKED="1", SDX_AUTOBUILD="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT, os.path.join(ROOT, "tests")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHECKED-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
