"""The BN3 fold HIP kernels (csrc/kernels/bnfold.hip) against the fp64 oracle of
tests/bnfold_oracle.py, bit for bit in the exact regime and within the derived bounds of
tests/bnfold_checks.py in the wide one (GPU). tests/test_bnfold_oracle.py shows on the CPU that
the bounds are reachable and sharp, that every named defect is caught and that each case sits on
the branch it is named for."""
import pytest
import torch

import bnfold_checks as K

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


def _report(stats):
    for k in sorted(stats):
        print(f"{k}: largest error / bound = {stats[k]:.4f}")


@pytest.mark.parametrize("regime", K.REGIMES)
@pytest.mark.parametrize("name", list(K.PREP_CASES))
def test_bnfold_prep(impl, name, regime):
    """Wd bit-equal, Mx bit-equal and symmetric (exact) or inside its bf16 interval (wide), b
    bit-equal or within its bound against the stored weights; no NaN; sentinels intact."""
    stats = {}
    K.check_prep(impl, name, regime, stats)
    _report(stats)


@pytest.mark.parametrize("regime", K.REGIMES)
@pytest.mark.parametrize("Kc,rows", K.COLSUM_CASES)
def test_bnfold_colsum(impl, Kc, rows, regime):
    """cs and every block's partial row, from a NaN-filled partial."""
    stats = {}
    K.check_colsum(impl, Kc, rows, regime, stats)
    _report(stats)


@pytest.mark.parametrize("regime", K.REGIMES)
@pytest.mark.parametrize("C,Kc,ncs,acc", K.WGRAD_CASES)
def test_bnfold_wgrad(impl, C, Kc, ncs, acc, regime):
    """accumulate = 0 overwrites a NaN-filled sink, accumulate = 1 updates a view inside a
    sentinel buffer in place; S is not symmetric."""
    stats = {}
    K.check_wgrad(impl, C, Kc, ncs, acc, regime, stats)
    _report(stats)


@pytest.mark.parametrize("kind", K.ROWDOT_KINDS)
@pytest.mark.parametrize("C,Kc,ns", K.ROWDOT_CASES)
def test_bnfold_rowdot(impl, C, Kc, ns, kind):
    """Sets 0 and 2 exactly 0 from a NaN-filled slab, hi in row 0 and lo in row 1 of set 1."""
    stats = {}
    K.check_rowdot(impl, C, Kc, ns, kind, stats)
    _report(stats)


def test_bnfold_repeatable(impl):
    K.check_repeatable(impl)


def test_bnfold_bindings_refuse(gpu):
    """Each call is refused (the launcher's hipErrorInvalidValue, or a binding check) before any
    launch: the outputs keep their sentinels."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()

    def f32(*shape):
        return torch.ones(*shape, device=gpu)

    def w(C, Kc):
        return torch.ones(C, 1, 1, Kc, device=gpu, dtype=BF16)

    def sent(n, dtype=torch.float32):
        return torch.full((n,), K.SENT, device=gpu, dtype=dtype)

    outs = []

    def prep(C, Kc, ldw, ldm):
        o = [sent(2 * Kc * max(C, ldw or C), BF16), sent(2 * Kc * max(Kc, ldm or Kc), BF16), sent(Kc)]
        outs.extend(o)
        return lambda: m.bnfold_prep(f32(3 * C), w(C, Kc), w(Kc, C), mu=f32(C), cs=f32(Kc), rows=64, ldw=ldw, ldm=ldm,
                                     wd_out=o[0], mx_out=o[1], bias_out=o[2])

    def colsum(Kc):
        o = sent(K.COLSUM_BLOCKS * Kc).view(K.COLSUM_BLOCKS, Kc)
        outs.append(o)
        return lambda: m.bnfold_colsum(torch.ones(16, Kc, device=gpu, dtype=BF16), partial=o)

    def rowdot(ns):
        o = sent(2 * ns * 8).view(2, ns, 8)
        outs.append(o)
        return lambda: m.bnfold_rowdot(f32(8, 16), w(8, 16), ns, o)

    small = sent(8 * 16 - 1)
    outs.append(small)
    refused = [(f"bnfold_prep {n}", prep(*a)) for n, a in K.PREP_REFUSED.items()] + \
              [(f"bnfold_colsum K = {Kc}", colsum(Kc)) for Kc in K.COLSUM_REFUSED] + \
              [(f"bnfold_rowdot ns = {ns}", rowdot(ns)) for ns in K.ROWDOT_REFUSED] + \
              [("bnfold_wgrad sink too small", lambda: m.bnfold_wgrad(f32(24), f32(8, 16), f32(16, 16), f32(1, 16),
                                                                    w(8, 16), small, True)),
               ("bnfold_wgrad no cs partial", lambda: m.bnfold_wgrad(f32(24), f32(8, 16), f32(16, 16), f32(0, 16),
                                                                   w(8, 16), f32(8, 16), True)),
               ("bnfold_prep wd_out too small", lambda: m.bnfold_prep(f32(24), w(8, 16), w(16, 8), wd_out=sent(127, BF16),
                                                                     mx_out=sent(256, BF16), bias_out=sent(16)))]
    for name, call in refused:
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"not refused: {name}")
    torch.cuda.synchronize()
    for o in outs:
        assert (o.float() == K.SENT).all(), "a refused call wrote to its output"
    # nothing above left an error behind: a valid call still runs
    cs, _ = m.bnfold_colsum(torch.ones(16, 8, device=gpu, dtype=BF16))
    assert cs.eq(16).all()
