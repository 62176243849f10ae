"""The native weighted k-NN kernels (csrc/kernels/knn.hip) against an fp64 CPU oracle, and
the evaluator on the native backend.

Similarity tolerance, derived: the bf16 hi/lo split drops at most 3·2^-18·Σ|a_i b_i| <= 3·2^-18
for unit rows, fp32 accumulation adds at most D·2^-24, so tol(D) = 3·2^-18 + D·2^-24. Order
statistics move by at most the sup-norm of a perturbation, so the sorted top-k values obey
the same bound with no excluded cases."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)

SHAPES = [(70, 1037, 512, 20), (64, 96, 2048, 96), (5, 300, 64, 1), (130, 2085, 2048, 200), (1, 257, 128, 256)]


def tol(D):
    return 3 * 2.0 ** -18 + D * 2.0 ** -24


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, d, generator=g, dtype=torch.float64), dim=1).float()


_CASES = {}


def _case(shape):
    """fp32 unit-norm inputs and their fp64 similarity matrix (computed once, never modified)."""
    if shape not in _CASES:
        nq, nb, d, k = shape
        q, b = _unit(nq, d, 100 + nq), _unit(nb, d, 200 + nb)
        sim = q.double() @ b.double().t()
        _CASES[shape] = (q, b, sim, torch.sort(sim, dim=1, descending=True).values[:, :k])
    return _CASES[shape]


def _check_topk(sims, idx, sim64, top64, nb, d):
    sims, idx = sims.cpu(), idx.cpu().long()
    assert sims.dtype == torch.float32 and tuple(sims.shape) == tuple(top64.shape) == tuple(idx.shape)
    assert bool((sims[:, 1:] <= sims[:, :-1]).all()), "rows must be non-increasing"
    e_sorted = float((sims.double() - top64).abs().max())
    assert int(idx.min()) >= 0 and int(idx.max()) < nb
    assert all(len(set(r)) == len(r) for r in idx.tolist()), "indices must be distinct per row"
    e_own = float((sim64.gather(1, idx) - sims.double()).abs().max())
    print(f"max |sims - oracle_sorted| {e_sorted:.3e}, max |oracle[idx] - sims| {e_own:.3e}, tol {tol(d):.3e}")
    assert e_sorted <= tol(d) and e_own <= tol(d)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_knn_topk_matches_fp64_oracle(gpu, shape):
    from simclr_pytorch_distributed_amd.ops.knn import knn_topk
    nq, nb, d, k = shape
    q, b, sim64, top64 = _case(shape)
    sims, idx = knn_topk(q.to(gpu), b.to(gpu), k)
    assert idx.dtype == torch.int32
    _check_topk(sims, idx, sim64, top64, nb, d)


def test_knn_topk_independent_of_splits_and_repeatable(gpu):
    from simclr_pytorch_distributed_amd.ops.knn import knn_topk
    nq, nb, d, k = SHAPES[0]
    q, b, _, _ = _case(SHAPES[0])
    q, b = q.to(gpu), b.to(gpu)
    s1, i1 = knn_topk(q, b, k, 1)
    for n_split in (3, 7):
        s, i = knn_topk(q, b, k, n_split)
        assert torch.equal(s, s1) and torch.equal(i, i1), n_split
    sa, ia = knn_topk(q, b, k)
    sb, ib = knn_topk(q, b, k)
    assert torch.equal(sa, sb) and torch.equal(ia, ib)
    assert torch.equal(sa, s1) and torch.equal(ia, i1)


def test_knn_topk_ties_go_to_the_lower_index(gpu):
    from simclr_pytorch_distributed_amd.ops.knn import knn_topk
    n = 150
    x = _unit(n, 128, 7)
    bank = torch.cat([x, x])
    q = _unit(37, 128, 8)
    k = (2 * n) // 2 + 3
    sims, idx = knn_topk(q.to(gpu), bank.to(gpu), k, 3)
    sims, idx = sims.cpu(), idx.cpu().long()
    both = 0
    for r in range(q.shape[0]):
        pos = {int(j): p for p, j in enumerate(idx[r].tolist())}
        for j in range(n):
            lo, hi = pos.get(j), pos.get(j + n)
            if lo is not None and hi is not None:
                both += 1
                assert sims[r, lo].view(torch.int32) == sims[r, hi].view(torch.int32), (r, j)
                assert lo < hi, (r, j)
            else:
                assert hi is None, f"query {r}: copy {j + n} returned without the lower index {j}"
    assert both > 0


@pytest.mark.parametrize("T", [0.1, 0.07])
@pytest.mark.parametrize("n_cls", [10, 100, 1000])
def test_knn_vote_scores_and_hits(gpu, n_cls, T):
    from simclr_pytorch_distributed_amd.ops.knn import knn_topk, knn_vote
    nq, nb, d, k = SHAPES[0]
    q, b, _, _ = _case(SHAPES[0])
    g = torch.Generator().manual_seed(n_cls)
    bank_labels = torch.randint(0, n_cls, (nb,), generator=g)
    labels = torch.randint(0, n_cls, (nq,), generator=g)
    sims, idx = knn_topk(q.to(gpu), b.to(gpu), k)
    scores, stats = knn_vote(sims, idx, bank_labels.to(gpu), n_cls, T, labels.to(gpu))
    # fp64 vote over the kernel's own lists
    want = torch.zeros(nq, n_cls, dtype=torch.float64)
    want.scatter_add_(1, bank_labels[idx.cpu().long()], torch.exp(sims.cpu().double() / T))
    got = scores.cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (nq, n_cls)
    assert bool(((got == 0) == (want == 0)).all()), "classes without a neighbour score exactly 0"
    nz = want > 0
    print("max rel err", float(((got.double() - want).abs()[nz] / want[nz]).max()))
    assert torch.allclose(got.double(), want, rtol=1e-4, atol=0.0)
    # hits recomputed in torch from the kernel's scores: rank = #{c: score_c > score_label}
    own = got.gather(1, labels[:, None])
    rank = (got > own).sum(dim=1)
    assert bool((own == 0).any()), "the case must include labels no neighbour voted for"
    assert stats.cpu().tolist() == [float((rank < 1).sum()), float((rank < 5).sum())]
    # without labels the scores are the same bits
    scores2, _ = knn_vote(sims, idx, bank_labels.to(gpu), n_cls, T)
    assert torch.equal(scores2, scores)


def test_knn_classify_backends(gpu):
    from simclr_pytorch_distributed_amd.ops.knn import knn_classify, knn_reference
    q, b = _unit(9, 96, 1).to(gpu), _unit(50, 96, 2).to(gpu)        # D = 96 is not 64·2^j
    bl = torch.randint(0, 5, (50,), generator=torch.Generator().manual_seed(3)).to(gpu)
    lab = torch.randint(0, 5, (9,), generator=torch.Generator().manual_seed(4)).to(gpu)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        knn_classify(q, b, bl, 5, k=10, T=0.1, backend="native")
    sc, st = knn_classify(q, b, bl, 5, k=10, T=0.1, labels=lab, backend="auto")
    ref, _, _ = knn_reference(q, b, bl, 5, 10, 0.1)
    assert torch.equal(sc, ref) and st.shape == (2,)
    # a supported shape through the public entry is the two kernels back to back
    from simclr_pytorch_distributed_amd.ops.knn import knn_topk, knn_vote
    q2, b2, _, _ = _case(SHAPES[0])
    q2, b2 = q2.to(gpu), b2.to(gpu)
    bl2 = torch.randint(0, 10, (b2.shape[0],), generator=torch.Generator().manual_seed(5)).to(gpu)
    sc2, none = knn_classify(q2, b2, bl2, 10, k=20, T=0.1, backend="native")
    want, _ = knn_vote(*knn_topk(q2, b2, 20), bl2, 10, 0.1)
    assert none is None and torch.equal(sc2, want)


def _synthetic(gpu, n_bank=256, n_val=128):
    from simclr_pytorch_distributed_amd.data.datasets import synthetic_dataset
    tr = synthetic_dataset(n_bank, 32, 10, 0, class_seed=0)
    va = synthetic_dataset(n_val, 32, 10, 1, class_seed=0)
    t = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    return t(tr.images), t(tr.labels), t(va.images), t(va.labels)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_evaluator_native(gpu, name):
    from simclr_pytorch_distributed_amd.data.augment import AugConfig, augment
    from simclr_pytorch_distributed_amd.data.store import DeviceStore
    from simclr_pytorch_distributed_amd.engine.knn import KnnEvaluator
    from simclr_pytorch_distributed_amd.models.resnet import SupConResNet
    from simclr_pytorch_distributed_amd.ops.linear_probe import FoldedEncoder
    torch.manual_seed(0)
    model = SupConResNet(name).to(gpu).to(memory_format=torch.channels_last)
    model.train()
    bx, by, vx, vy = _synthetic(gpu)
    bank = DeviceStore(bx, by)
    ev = KnnEvaluator(model, "native", "bf16", bank, DeviceStore(vx, vy), AugConfig.evaluation(32, MEAN, STD), 10,
                      k=200, T=0.1, batch_size=128)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    top1, top5 = ev.evaluate()
    assert 0.0 <= top1 <= top5 <= 100.0
    assert model.training and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    x = augment(bx, torch.arange(128, device=gpu), AugConfig.evaluation(32, MEAN, STD), 0)
    direct = F.normalize(FoldedEncoder(model.encoder)(x).float(), dim=1)
    assert ev.last_bank.shape == (256, 512 if name == "resnet18" else 2048)
    assert torch.equal(ev.last_bank[:128], direct)
    assert torch.equal(ev.extract(bank, 0, 128), direct)


def test_evaluate_leaves_training_undisturbed(gpu, tmp_path):
    """Two engines from one seed; one evaluates between step 1 and step 2: step 2's loss and the
    updated flat parameter buffer are bit-identical."""
    from simclr_pytorch_distributed_amd.config import parse_pretrain
    from simclr_pytorch_distributed_amd.engine.pretrain import PretrainEngine
    res = []
    for knn_freq in (0, 1):
        opt = parse_pretrain(["--batch_size", "32", "--synthetic", "--synthetic_size", "128", "--work_dir",
                              str(tmp_path / f"k{knn_freq}"), "--model", "resnet18", "--backend", "native",
                              "--learning_rate", "0.05", "--seed", "3", "--knn_freq", str(knn_freq), "--knn_k", "50"],
                             make_dirs=False)
        eng = PretrainEngine(opt)
        eng.model.train()
        idx = torch.arange(32, device=gpu)
        eng.train_step(idx, 1, 0, 10)
        if knn_freq:
            seed, rng = eng._seed_host, torch.get_rng_state()
            top1, top5 = eng.knn.evaluate()
            assert 0.0 <= top1 <= top5 <= 100.0
            assert eng._seed_host == seed and torch.equal(torch.get_rng_state(), rng) and eng.model.training
        st = eng.train_step(idx + 32, 1, 1, 10)
        torch.cuda.synchronize()
        res.append((st["loss_local"].clone(), eng.flat.flat.clone(), eng.optimizer.buf.clone(),
                    [b.clone() for b in eng.model.buffers()]))
    (l0, w0, m0, b0), (l1, w1, m1, b1) = res
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert torch.equal(w0, w1) and torch.equal(m0, m1)
    assert all(torch.equal(a, b) for a, b in zip(b0, b1))


CHECKED_SCRIPT = r"""
import torch, torch.nn.functional as F
from simclr_pytorch_distributed_amd.ops import _ext
m = _ext.require()
assert m.__name__.endswith("_C_checked"), m.__name__
g = torch.Generator().manual_seed(0)
q = F.normalize(torch.randn(70, 512, generator=g, dtype=torch.float64), dim=1).float()
b = F.normalize(torch.randn(1037, 512, generator=g, dtype=torch.float64), dim=1).float()
for n_split in (0, 1, 3):
    sims, idx = m.knn_topk(q.cuda(), b.cuda(), 20, n_split)
    want = torch.sort(q.double() @ b.double().t(), dim=1, descending=True).values[:, :20]
    assert float((sims.cpu().double() - want).abs().max()) <= 3 * 2.0 ** -18 + 512 * 2.0 ** -24
lab = torch.randint(0, 10, (1037,), generator=g).cuda()
m.knn_vote(sims, idx, lab, 10, 0.1, torch.randint(0, 10, (70,), generator=g).cuda())
torch.cuda.synchronize()
print("CHECKED-OK")
"""


def test_knn_checked_build_runs_clean(gpu):
    if not os.path.exists(os.path.join(ROOT, "simclr_pytorch_distributed_amd", "_C_checked.so")):
        pytest.skip("checked build not present (python csrc/build.py --checked)")
    env = dict(os.environ, SDX_CHECKED="1", SDX_AUTOBUILD="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHECKED_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHECKED-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
