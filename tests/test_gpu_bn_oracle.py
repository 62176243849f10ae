"""The BatchNorm HIP kernels (csrc/kernels/bn.hip, csrc/include/bn_epilogue.h) against the
fp64 oracle of tests/bn_oracle.py at the edge shapes and within the derived bounds of
tests/bn_checks.py (GPU). tests/test_bn_oracle.py shows on the CPU that the bounds are reachable
and sharp and that each case sits on the path it is named for."""
import os
import subprocess
import sys

import pytest
import torch

import bn_checks as K

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


def _report(stats):
    for k in sorted(stats):
        print(f"{k}: largest error / bound = {stats[k]:.4f}")


@pytest.mark.parametrize("C,rows", K.EW_CASES + K.EW_KNOB_CASES)
def test_bn_apply(impl, C, rows):
    """Every res mode, ReLU on and off, with and without mask_out."""
    stats = {}
    K.check_apply(impl, C, rows, stats)
    _report(stats)


@pytest.mark.parametrize("C,rows", K.EW_CASES + K.EW_KNOB_CASES)
def test_bn_bwd_apply(impl, C, rows):
    """One and two sets, each mask source, want_dz on and off; dz bit-equal."""
    stats = {}
    K.check_bwd_apply(impl, C, rows, stats)
    _report(stats)


@pytest.mark.parametrize("C,rows", K.REDUCE_CASES)
def test_bn_bwd_reduce_and_coef(impl, C, rows):
    """bn_bwd_reduce, bn_bwd_coef (exact sums, grad_scale 0.25) and bn_bwd_reduce_coef (bit-equal
    to the two, three calls in a row): one and two sets, each mask source, sinks given and absent."""
    stats = {}
    K.check_bwd_reduce(impl, C, rows, stats)
    _report(stats)


@pytest.mark.parametrize("g", K.REDUCE3_G)
def test_bn_bwd_reduce_three_sets(impl, g):
    """Two BN sets with a partial slab of g rows: the 3-set column reduction (plain and with the
    coefficient epilogue) on the row table of the column reduction; bn_bwd_reduce within its
    bound, bn_bwd_reduce_coef bit-equal to reduce + coef over three calls and within the
    composed bound, sinks given and absent."""
    stats = {}
    K.check_bwd_reduce3(impl, g, stats)
    _report(stats)


@pytest.mark.parametrize("C", K.STATS_C)
def test_bn_stats_reduce_finalize(impl, C):
    """bn_stats_reduce, bn_finalize and bn_stats_finalize (bit-equal to the two, three calls in
    a row) at the row counts around every edge of the column reduction."""
    stats = {}
    for rows in K.stats_rows_for(C):
        K.check_stats(impl, rows, C, stats)
    _report(stats)


def test_bn_finalize_edges(impl):
    stats = {}
    K.check_finalize_edges(impl, stats)
    _report(stats)


def test_bn_eval_affine(impl):
    """Measured tolerance (rsqrtf): within twice the recorded error of the fp64 oracle, which
    itself may not pass 8·2^-24; chained through bn_apply, the bn_apply bound holds."""
    stats = {}
    worst = max(K.eval_affine_error(impl, C) for C in K.EVAL_CASES)
    print(f"bn_eval_affine: largest relative error = {worst / K.U24:.4f} x 2^-24")
    assert worst <= K.EVAL_AFFINE_CEILING, "beyond 8·2^-24 the error is not rounding"
    assert worst <= K.EVAL_AFFINE_TOL
    for C in K.EVAL_CASES:
        K.check_eval_chain(impl, C, stats)
    _report(stats)


def test_bn_bindings_refuse(gpu):
    """Host checks only: each call is refused by the binding before any launch."""
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()

    def act(C, rows=4):
        return torch.zeros(1, 1, rows, C, device=gpu).bfloat16()

    def vec(C):
        return torch.ones(C, device=gpu)

    refused = [
        ("bn_bwd_reduce C = 24 (check_bwd_C)", lambda: m.bn_bwd_reduce(act(24), None, act(24), vec(24))),
        ("bn_bwd_reduce C = 4096 (check_bwd_C)", lambda: m.bn_bwd_reduce(act(4096), None, act(4096), vec(4096))),
        ("bn_bwd_reduce_coef C = 24", lambda: m.bn_bwd_reduce_coef(act(24), None, act(24), vec(24), count=4.0,
                                                                   g_a=vec(24), inv_a=vec(24))),
        ("bn_apply C = 12 (check_bf16_nhwc)", lambda: m.bn_apply(act(12), vec(12), vec(12), None, None, None, 0, True)),
        ("slab C = 4104, bn_stats_reduce (check_slab)", lambda: m.bn_stats_reduce(torch.zeros(4, 2, 4104, device=gpu))),
        ("slab C = 4104, bn_stats_finalize (check_slab)",
         lambda: m.bn_stats_finalize(torch.zeros(4, 2, 4104, device=gpu), 64.0, None, None, 1e-5, 0.1, False, None, None)),
        ("bn_apply mask_out of the wrong length (check_mask)",
         lambda: m.bn_apply(act(16), vec(16), vec(16), None, None, None, 0, True,
                            mask_out=torch.zeros(4 * 16 // 8 + 1, dtype=torch.uint8, device=gpu))),
        ("bn_apply res_mode 1 without scale2", lambda: m.bn_apply(act(16), vec(16), vec(16), act(16), None, vec(16), 1, True)),
        ("bn_bwd_coef sums [1, C]", lambda: m.bn_bwd_coef(torch.zeros(1, 16, dtype=torch.float64, device=gpu), 4.0,
                                                         vec(16), vec(16), vec(16))),
        ("bn_stats_reduce of an empty slab", lambda: m.bn_stats_reduce(torch.zeros(0, 2, 16, device=gpu))),
    ]
    for name, call in refused:
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"not refused: {name}")
    torch.cuda.synchronize()
    # nothing above left an error behind: a valid call still runs
    assert m.bn_stats_reduce(torch.ones(3, 2, 16, device=gpu)).eq(3).all()


def test_bn_knobs_in_a_fresh_process(gpu):
    """SDX_EW_BLOCKS / SDX_EW_BLOCKS_BWD / SDX_CR_GY are read once per process, so the small
    cases run again in one fresh child under non-default values (several grid-stride iterations,
    gy = 12 with empty trailing blocks at 9 rows) through the same comparison functions."""
    env = dict(os.environ, SDX_AUTOBUILD="0", PYTHONPATH=os.pathsep.join([ROOT, TESTS]), **K.KNOB_ENV)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "bn_checks.py"), "--child"], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and K.CHILD_MARKER in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
