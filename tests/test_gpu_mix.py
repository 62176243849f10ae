"""The mixing kernel (csrc/kernels/mix.hip), the soft-target forward ops (ce_head_fwd_soft,
ce_head_fwd_soft_mfma), the autograd node and the native engine with --mixup / --cutmix /
--label_smoothing, against tests/mix_oracle.py under the bounds derived in tests/mix_checks.py.

Worst error / bound seen on an MI355X: see docs/PARITY.md ("Beyond the reference").
"""
import os
import subprocess
import sys

import pytest
import torch

import mix_checks as MC
import mix_oracle as MO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m():
    from simclr_pytorch_distributed_amd.ops import _ext
    return _ext.require()


def _mix(x, mode, lam, box=(0, 0, 0, 0), out=None):
    from simclr_pytorch_distributed_amd.data.augment import mix_views
    return mix_views(x, mode, lam, *box, out=out)


# ---- mix_views ---------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 7, 32])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_cutmix_is_a_bit_copy(gpu, B, S):
    x = MC.batch(B, S)
    xd = x.to(gpu)
    keep = xd.clone()
    for name, box in MC.boxes(S).items():
        got = _mix(xd, "cutmix", 0.5, box)
        assert got.data_ptr() != xd.data_ptr()
        MC.check_cutmix(got.cpu(), x, box, f"B={B} S={S} {name}")
    assert torch.equal(xd.view(torch.int16), keep.view(torch.int16))        # the input is left untouched


def test_cutmix_grid_stride_224(gpu):
    """3 x 224² = 150528 pixels over the capped grid of 512 x 256 threads: some threads take two."""
    x = MC.batch(3, 224, seed=1)
    for box in ((0, 224, 0, 224), (17, 190, 100, 101), (223, 224, 0, 224)):
        MC.check_cutmix(_mix(x.to(gpu), "cutmix", 0.5, box).cpu(), x, box, f"224 {box}")
    MC.check_mixup_wide(_mix(x.to(gpu), "mixup", 0.3).cpu(), x, 0.3, "224")


@pytest.mark.parametrize("B,S", [(1, 1), (2, 7), (5, 32)])
def test_mixup_exact_regime(gpu, B, S):
    x = MC.batch(B, S, exact=True)
    for lam in (0.25, 0.5, 0.75):
        MC.check_mixup_exact(_mix(x.to(gpu), "mixup", lam).cpu(), x, lam, f"B={B} S={S} lam={lam}")


@pytest.mark.parametrize("B,S", [(1, 7), (2, 1), (5, 32)])
def test_mixup_wide_regime(gpu, B, S):
    x = MC.batch(B, S)
    g = torch.Generator().manual_seed(B + S)
    worst = 0.0
    for lam in [0.3] + torch.rand(4, generator=g).tolist():
        worst = max(worst, MC.check_mixup_wide(_mix(x.to(gpu), "mixup", lam).cpu(), x, lam, f"B={B} S={S} lam={lam}"))
    print(f"mixup wide B={B} S={S}: largest (|stored - s| - half ulp) / delta = {worst:.3f}")
    # λ = 1 and λ = 0 reproduce x and its roll numerically (a −0 may come back +0)
    assert torch.equal(_mix(x.to(gpu), "mixup", 1.0).cpu().float(), x.float())
    assert torch.equal(_mix(x.to(gpu), "mixup", 0.0).cpu().float(), x.roll(1, 0).float())


def test_mix_views_refusals_leave_the_output_untouched(gpu):
    m = _m()
    x = MC.batch(2, 7).to(gpu)
    out = torch.full_like(x, 3.0)
    bad = [
        (x.float(), 2, 0.5, 0, 1, 0, 1),                             # not bf16
        (x[:, :, ::2], 2, 0.5, 0, 1, 0, 1),                          # not contiguous
        (x[..., :4].contiguous(), 2, 0.5, 0, 1, 0, 1),               # last dimension != 8
        (x[:0], 2, 0.5, 0, 0, 0, 0),                                 # empty batch
        (x, 2, 0.5, 0, 8, 0, 1), (x, 2, 0.5, -1, 1, 0, 1), (x, 2, 0.5, 3, 2, 0, 1), (x, 2, 0.5, 0, 1, 5, 9),   # box
        (x, 1, 1.5, 0, 0, 0, 0), (x, 1, -0.1, 0, 0, 0, 0), (x, 2, float("nan"), 0, 1, 0, 1),                  # λ
        (x, 0, 0.5, 0, 0, 0, 0), (x, 3, 0.5, 0, 0, 0, 0),            # mode
    ]
    for args in bad:
        o = out if args[0].shape == out.shape and args[0].dtype == out.dtype else torch.full_like(args[0], 3.0)
        with pytest.raises(RuntimeError):
            m.mix_views(*args, o)
        torch.cuda.synchronize()
        assert bool((o.float() == 3.0).all()), args[1:]
    with pytest.raises(RuntimeError):
        m.mix_views(x, 1, 0.5, 0, 0, 0, 0, x)                         # in place
    with pytest.raises(RuntimeError):
        m.mix_views(x, 1, 0.5, 0, 0, 0, 0, out.float())
    got = m.mix_views(x, 2, 0.5, 0, 7, 0, 7, out)                     # and a good call fills `out`
    assert got.data_ptr() == out.data_ptr() and torch.equal(out.cpu().float(), x.roll(1, 0).cpu().float())


# ---- soft cross-entropy --------------------------------------------------------------------------

def _ops(gemm):
    m = _m()
    return (m.ce_head_fwd_soft_mfma, m.ce_head_fwd_mfma, m.ce_head_bwd_mfma) if gemm == "mfma" else \
        (m.ce_head_fwd_soft, m.ce_head_fwd, m.ce_head_bwd)


def _check_sums(ctx, rowstat, stats, loss):
    """stats = (float) of the fp64 row-order sums of the implementation's own rowstat, loss = (float)(Σ / B)."""
    sums = [0.0, 0.0, 0.0]
    for row in rowstat.double().cpu().tolist():
        sums = [s + v for s, v in zip(sums, row)]
    want = torch.tensor(sums + [sums[0] / rowstat.shape[0]], dtype=torch.float64).float().nan_to_num(-7.0)
    got = torch.cat([stats.cpu(), loss.cpu().view(1)]).nan_to_num(-7.0)
    assert torch.equal(got, want), f"{ctx}: stats / loss"


def _soft_sweep(gpu, gemm, K, C, Bs, worst):
    soft, plain, _ = _ops(gemm)
    for B in Bs:
        for exact in (False, True):
            x, W, b, la, lb = MC.ce_inputs(B, K, C, exact=exact)
            xd, Wd, bd = x.to(gpu), W.to(gpu), b.to(gpu)
            z_plain = plain(xd, Wd, bd, la.to(gpu), True)[0]
            la, lb = MC.plant_labels(z_plain.cpu(), la, lb)
            for lam in (0.0, 0.3, 0.5, 1.0):
                for eps in (0.0, 0.1):
                    ctx = f"{gemm} B={B} K={K} C={C} lam={lam} eps={eps} exact={exact}"
                    logits, dz, rowstat, stats, loss = soft(xd, Wd, bd, la.to(gpu), lb.to(gpu), lam, eps, True)
                    assert torch.equal(logits, z_plain), f"{ctx}: logits differ from the plain op's"
                    # (exact regime: the logits are small integers and halves, ties included; the hits
                    # are the oracle's on them exactly)
                    MC.check_soft(worst, ctx, logits.cpu(), la, lb, lam, eps, MC.f32(1.0 / B), rowstat.cpu(), dz.cpu())
                    _check_sums(ctx, rowstat, stats, loss)


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("C", [1, 3, 5, 65, 1000])
def test_soft_ce_fma(gpu, K, C):
    worst = MC.Worst()
    _soft_sweep(gpu, "fma", K, C, (1, 4, 5, 37), worst)
    print(f"soft CE fma K={K} C={C}: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("K", [192, 2048])
@pytest.mark.parametrize("C", [3, 65, 1000])
def test_soft_ce_mfma(gpu, K, C):
    worst = MC.Worst()
    _soft_sweep(gpu, "mfma", K, C, (1, 5, 37), worst)
    print(f"soft CE mfma K={K} C={C}: worst error / bound {worst.ratio:.3f} at {worst.where}")


@pytest.mark.parametrize("B,K,C", [(5, 64, 10), (37, 256, 1000)])
def test_soft_ce_fma_against_fp64_torch_on_the_inputs(gpu, B, K, C):
    """The rule of tests/test_gpu_ce_head.py (4 x fp32 torch's own error + one fp32 ulp of the
    magnitude), extended by the derived target terms of mix_checks: loss and dz."""
    import torch.nn.functional as F
    x, W, b, la, lb = MC.ce_inputs(B, K, C)
    lam, eps = 0.3, 0.1
    t64 = MO.soft_target(la, lb, MC.f32(lam), MC.f32(eps), C)

    def torch_ce(dtype):
        z = F.linear(x.to(dtype), W.to(dtype), b.to(dtype)).requires_grad_(True)
        loss = F.cross_entropy(z, t64.to(dtype))
        return loss.detach().double(), torch.autograd.grad(loss, [z])[0].double()

    (l64, d64), (l32, d32) = torch_ce(torch.float64), torch_ce(torch.float32)
    logits, dz, rowstat, stats, loss = _m().ce_head_fwd_soft(x.to(gpu), W.to(gpu), b.to(gpu), la.to(gpu), lb.to(gpu),
                                                             lam, eps, True)
    Bd = MC.soft_bounds(logits.cpu(), la, lb, lam, eps, MC.f32(1.0 / B))
    for q, got, r64, r32, extra in (("loss", loss.double().cpu(), l64, l32, float(Bd["tgt"].mean())),
                                    ("dz", dz.double().cpu(), d64, d32, float(Bd["dt"].max()) / B)):
        e32, ek = float((r32 - r64).abs().max()), float((got - r64).abs().max())
        allow = 4.0 * e32 + 2.0 ** -23 * float(r64.abs().max()) + extra
        print(f"B={B} K={K} C={C} {q}: kernel err {ek:.3e}, fp32 torch err {e32:.3e}, allowed {allow:.3e}, "
              f"ratio {ek / allow:.3f}")
        assert ek <= allow, q


@pytest.mark.parametrize("gemm,K,C", [("fma", 64, 5), ("fma", 256, 1000), ("mfma", 192, 65), ("mfma", 2048, 1000)])
@pytest.mark.parametrize("final", [False, True])
def test_soft_reduces_to_plain_bit_for_bit(gpu, gemm, K, C, final):
    soft, plain, bwd = _ops(gemm)
    for B in (1, 5, 37):
        x, W, b, la, _ = (t.to(gpu) for t in MC.ce_inputs(B, K, C))
        if B >= 4:
            la[B - 1] = -1
        p = plain(x, W, b, la, final)
        s = soft(x, W, b, la, la.clone(), 1.0, 0.0, final)
        if not final:       # the backward op sums the statistics
            one = torch.ones((), device=gpu)
            for o in (p, s):
                bwd(x, o[1], W, one, o[2], o[3], o[4], None, None, True)
        torch.cuda.synchronize()
        for name, u, v in zip(("logits", "dz", "rowstat", "stats", "loss"), p, s):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{gemm} B={B} K={K} C={C}: {name}"


@pytest.mark.parametrize("gemm,K,C", [("fma", 256, 65), ("mfma", 192, 65)])
def test_soft_node_through_autograd(gpu, gemm, K, C):
    """classifier_ce with a soft target + backward() = the backward op called by hand on the soft
    forward's dz, bit for bit; two runs are bit-identical."""
    from simclr_pytorch_distributed_amd.ops.ce_head import classifier_ce_logits
    soft, _, bwd = _ops(gemm)
    B = 37
    x, W, b, la, lb = (t.to(gpu) for t in MC.ce_inputs(B, K, C))

    def run():
        fc = torch.nn.Linear(K, C).to(gpu)
        with torch.no_grad():
            fc.weight.copy_(W)
            fc.bias.copy_(b)
        xr = x.clone().requires_grad_(True)
        loss, stats, logits = classifier_ce_logits(xr, fc, la, gemm=gemm, labels2=lb, lam=0.3, smoothing=0.1)
        assert type(loss.grad_fn).__name__.startswith("_ClassifierCE")
        loss.backward()
        torch.cuda.synchronize()
        return [loss.detach(), stats, logits, xr.grad, fc.weight.grad, fc.bias.grad]

    r1, r2 = run(), run()
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    logits, dz, rowstat, stats, loss = soft(x, W, b, la, lb, 0.3, 0.1, False)
    dW, db = torch.zeros_like(W), torch.zeros_like(b)
    dX = bwd(x, dz, W, torch.ones((), device=gpu), rowstat, stats, loss, dW, db, True)
    torch.cuda.synchronize()
    for name, u, v in zip(("loss", "stats", "logits", "dX", "dW", "db"), r1, [loss, stats, logits, dX, dW, db]):
        assert torch.equal(u, v), name
    ref = MO.soft_ce(logits.cpu(), la.cpu(), lb.cpu(), MC.f32(0.3), MC.f32(0.1), 1.0 / B)
    assert abs(float(loss) - float(ref["loss"].mean())) < 1e-5


# ---- native engine -------------------------------------------------------------------------------

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


MIX_FLAGS = ("--mixup", "0.8", "--cutmix", "1.0", "--label_smoothing", "0.1")


def _run_steps(eng, epoch, n=2):
    eng.model.train()
    out = []
    for it, (idx, labels) in enumerate(eng.epoch_batches(epoch)):
        if it >= n:
            break
        out.append((eng.train_step(idx, labels, epoch, it, n), labels))
    torch.cuda.synchronize()
    return out


def test_native_engine_mixes_by_the_draw(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.data.augment import mix_draw
    eng = _engine(tmp_path, gpu, *MIX_FLAGS)
    spy = _Spy(monkeypatch, "mix_views", "ce_head_fwd_soft", "ce_head_fwd")
    steps = _run_steps(eng, 1)
    assert len(spy.calls["mix_views"]) == 2 and len(spy.calls["ce_head_fwd_soft"]) == 2 and not spy.calls["ce_head_fwd"]
    for it, ((st, labels), (margs, _), (cargs, cres)) in enumerate(zip(steps, spy.calls["mix_views"],
                                                                      spy.calls["ce_head_fwd_soft"])):
        mode, lam, box = mix_draw(eng.opt, eng.opt.seed, 1, it, 0)
        assert mode != "none"
        assert margs[1:7] == ({"mixup": 1, "cutmix": 2}[mode], lam, *box) and tuple(margs[0].shape) == (8, 32, 32, 8)
        a, b = (labels, labels.roll(1)) if lam >= 0.5 else (labels.roll(1), labels)
        assert torch.equal(cargs[3], a) and torch.equal(cargs[4], b)
        assert cargs[5] == (lam if lam >= 0.5 else 1.0 - lam) and cargs[6] == 0.1
        logits = cres[0].cpu()
        Bd = MC.soft_bounds(logits, a.cpu(), b.cpu(), cargs[5], 0.1, MC.f32(1.0 / 8))
        want = float(Bd["ref"]["loss"].mean())
        assert abs(float(st["loss_local"]) - want) <= float(Bd["row"].mean()) + MC.U * abs(want), it


def test_native_engine_flags_absent_is_todays_step(gpu, tmp_path, monkeypatch):
    from simclr_pytorch_distributed_amd.engine.supervised import SupervisedEngine
    a = _engine(tmp_path / "a", gpu)
    spy = _Spy(monkeypatch, "mix_views", "ce_head_fwd_soft", "ce_head_fwd_soft_mfma")
    (sa, _), = _run_steps(a, 1, 1)
    assert not any(spy.calls.values())
    monkeypatch.setattr(SupervisedEngine, "_mix", lambda *args: pytest.fail("the mixing code ran"))
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


def test_native_engine_resume_repeats_the_draws(gpu, tmp_path, monkeypatch):
    eng = _engine(tmp_path, gpu, *MIX_FLAGS, "--epochs", "1")
    last = eng.run()
    spy = _Spy(monkeypatch, "mix_views")
    _run_steps(eng, 2)                                   # the uninterrupted run's epoch 2
    straight = [c[0][1:7] for c in spy.calls["mix_views"]]
    spy.calls["mix_views"].clear()
    eng2 = _engine(tmp_path, gpu, *MIX_FLAGS, "--epochs", "2", "--resume", last)
    assert eng2.start_epoch == 2
    _run_steps(eng2, 2)
    assert len(straight) == 2 and [c[0][1:7] for c in spy.calls["mix_views"]] == straight


# ---- checked build -------------------------------------------------------------------------------

CHECKED_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from simclr_pytorch_distributed_amd.ops import _ext
m = _ext.require()
assert m.__name__.endswith("_C_checked")
import mix_checks as MC
x = MC.batch(3, 224).cuda()
m.mix_views(x, 1, 0.3, 0, 0, 0, 0, None)
m.mix_views(x, 2, 0.5, 17, 190, 0, 224, None)
m.mix_views(MC.batch(1, 1).cuda(), 2, 0.5, 0, 1, 0, 1, None)
for op, K in ((m.ce_head_fwd_soft, 256), (m.ce_head_fwd_soft_mfma, 192)):
    a, W, b, la, lb = (t.cuda() for t in MC.ce_inputs(37, K, 1000))
    la[36] = -1
    op(a, W, b, la, lb, 0.3, 0.1, True)
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
