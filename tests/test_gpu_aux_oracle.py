"""The max-pool (csrc/kernels/pool.hip), weight-prep (wprep.hip) and linear-probe step
(linear_ce.hip, one case of linear_ce_sweep.hip) HIP kernels against the fp64 oracles of
tests/aux_oracle.py: bit for bit wherever the operation is integer-exact or one rounding, within
the derived bounds of tests/aux_checks.py elsewhere (GPU). tests/test_aux_oracle.py shows on the
CPU that the oracles agree with float64 torch, that the guards hold and that every named defect
is caught."""
import pytest
import torch

import aux_checks as K

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


def _report(stats):
    for k in sorted(stats):
        print(f"{k}: largest error / bound = {stats[k]:.4f}")


@pytest.mark.parametrize("name", list(K.POOL_CASES))
def test_maxpool(impl, name):
    """y (but for the sign of a zero) and idx as the oracle's; with dy in halves both backwards
    bit-equal to the oracle and to each other, uncovered inputs exactly 0; with random dy the
    stored bf16 inside its interval. The -inf cases hold edge windows that are all -inf."""
    stats, tally = {}, {}
    K.check_pool(impl, name, stats, tally)
    _report(stats)
    print("windows whose maximum is a zero of either sign:", tally)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_maxpool_grid_stride(impl, which):
    """1 114 112 eight-channel groups: one full trip of the 4096 x 256 grid and a partial one."""
    K.check_pool_grid(impl, which)


def test_maxpool_bindings_refuse(gpu):
    """stride < 1, k < 1, a y that is not [N, P, Q, C] of x and the geometry: refused before a
    launch; nothing is returned and the sentinel-filled tensors stay as they were."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    kept = []

    def sent(shape, dtype=BF16):
        t = torch.full(shape, 7 if dtype == torch.uint8 else K.SENT, device=gpu, dtype=dtype)
        kept.append((t, t.clone()))
        return t

    for name, xs, ys, k, s, p in K.POOL_REFUSED:
        x = sent(xs)
        if ys is None:
            ys = (xs[0], 4, 4, xs[3])
            calls = [lambda: m.maxpool_fwd(x, k, s, p), lambda: m.maxpool_fwd_idx(x, k, s, p),
                     lambda: m.maxpool_bwd_idx(sent(ys, torch.uint8), sent(ys), xs[1], xs[2], k, s, p)]
        else:
            calls = []
        calls.append(lambda: m.maxpool_bwd(x, sent(ys), sent(ys), k, s, p))
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
                pytest.fail(f"not refused: {name}")
    with pytest.raises(RuntimeError):                      # dy of another shape than y
        m.maxpool_bwd(sent((1, 8, 8, 8)), sent((1, 4, 4, 8)), sent((1, 4, 4, 16)), 3, 2, 1)
    torch.cuda.synchronize()
    for t, before in kept:
        assert torch.equal(t, before), "a refused call wrote to a tensor"
    assert m.maxpool_fwd(torch.ones(1, 8, 8, 8, device=gpu, dtype=BF16), 3, 2, 1).eq(1).all()   # no error left behind


@pytest.mark.parametrize("name", list(K.WPREP_TABLES))
def test_wprep(impl, gpu, name):
    """Every 16-bit pattern of the sentinel-filled output buffer after one launch over the
    production segment table of toy modules: slices, zero padding, alignment gaps."""
    K.check_wprep(impl, name, gpu)


@pytest.mark.parametrize("rows,Cp,C", K.UNPAD_CASES)
def test_unpad_add(impl, rows, Cp, C):
    K.check_unpad_add(impl, rows, Cp, C)


@pytest.mark.parametrize("Kc", K.PROBE_K)
def test_probe_forward_exact(impl, Kc):
    """Every KJ instantiation x C in {1, 3, 5, 64, 65, 1000, 1024} x B in {1, 4, 5, 37}: logits
    bit-equal, hits by the strict-greater rule with the label level with the maximum and with
    5th place, labels -1 and C: NaN loss, no hit, dz the plain softmax / B."""
    stats = {}
    for C in K.PROBE_C:
        for B in K.PROBE_B:
            K.check_probe_fwd_exact(impl, Kc, C, B, stats)
    _report(stats)


@pytest.mark.parametrize("C,Kc,B,first,wd", K.SGD_CASES)
def test_probe_sgd_exact(impl, C, Kc, B, first, wd):
    """linear_ce_sgd_raw on integers and signed powers of two: W, b, both momentum buffers (views
    inside a sentinel buffer) and stats bit-equal, the bias decay and the first-step rule included."""
    K.check_sgd_exact(impl, C, Kc, B, first, wd)


@pytest.mark.parametrize("Kc", K.PROBE_WIDE_K)
def test_probe_wide(impl, Kc):
    """K = 128, 256, 1024 on random fp32: loss, logits, dz by the rule of test_gpu_ce_head.py; three
    SGD steps (lr 30, 0.5, 0.01) from the kernel's own dz within the derived bound."""
    stats = {}
    for C, B in K.PROBE_WIDE_CB:
        K.check_probe_wide(impl, Kc, C, B, stats)
        K.check_sgd_wide(impl, Kc, C, B, stats)
    _report(stats)


def test_probe_sweep_and_eval(impl):
    """One sweep case straight against the oracle (G = 3, K = 256), and the statistics-only call
    of linear_ce_step, which leaves the parameter views untouched."""
    K.check_sweep(impl)
    for Kc, C, B in ((256, 65, 5), (64, 3, 1)):
        K.check_eval_untouched(impl, Kc, C, B)
