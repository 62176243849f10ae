"""The convolution HIP kernels (csrc/include/igemm_kernel.h, csrc/kernels/wgrad1x1.hip,
wgrad3x3.hip, splitk.hip) against the fp64 oracle of tests/conv_oracle.py on integer inputs:
y, dx, dW and every exact statistic bit for bit, Σy² past 2^24 within its derived bound
(tests/conv_checks.py). tests/test_conv_oracle.py shows on the CPU that the comparisons catch
each defect they are meant for and that each case sits on the path it is named for."""
import os
import subprocess
import sys

import pytest
import torch

import conv_checks as K

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
TAP_SHAPES = [(n, h, h, c, k, 3, 1, 1) for n, h, c, k in K.TAP_CASES]


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


@pytest.mark.parametrize("name", list(K.FWD_CASES))
def test_fwd_and_dgrad(impl, name):
    """Auto dispatch and every pinned tile config, both regimes; the single-stage case at both
    igemm_one_k_set limits of each pass."""
    shape = K.FWD_CASES[name]
    limits = {0: (64, 4096), 1: (32, 4096)} if name == "single-stage DEPTH 3" else {0: (None,), 1: (None,)}
    for mode, check in ((0, K.check_fwd), (1, K.check_dgrad)):
        for lim in limits[mode]:
            prev = impl.m.igemm_one_k_set(mode, lim) if lim is not None else None
            try:
                for regime in K.REGIMES:
                    for cfg in K.PINNED_CFGS:
                        check(impl, shape, regime, cfg)
            finally:
                if lim is not None:
                    impl.m.igemm_one_k_set(mode, prev)


@pytest.mark.parametrize("shape", TAP_SHAPES)
def test_tap_tiles(impl, shape):
    """Tap-reuse tiles 11-13: forward, data gradient, data gradient with statistics."""
    for regime in K.REGIMES:
        K.check_fwd(impl, shape, regime)
        K.check_dgrad(impl, shape, regime)
        for mask in K.MASKS:
            K.check_dgrad_bnstat(impl, shape, regime, mask=mask)
        K.check_dgrad_bnstat(impl, shape, regime, sets=2, mask="bits", addend="masked")


@pytest.mark.parametrize("regime", K.REGIMES)
def test_epilogues(impl, regime):
    """conv_fwd_bias, the operand prologue of forward and wgrad, the addend forms, conv_dgrad_cat."""
    for shape in K.BIAS_SHAPES:
        for relu in (True, False):
            K.check_fwd_bias(impl, shape, regime, relu)
    for shape in K.EPI_SHAPES:
        for cfg in (-1, 0, 3):
            K.check_fwd(impl, shape, regime, cfg, prologue=True)
            K.check_wgrad(impl, shape, regime, cfg if cfg >= 0 else -2, 0, prologue=True)
            K.check_wgrad(impl, shape, regime, cfg if cfg >= 0 else -2, 2, "krsc", prologue=True)
            for a in K.ADDENDS[1:]:
                K.check_dgrad(impl, shape, regime, cfg, a)
    for case in K.CAT_CASES:
        for cfg in (-1, 1, 4, 6):
            K.check_dgrad_cat(impl, case, regime, cfg)


@pytest.mark.parametrize("shape", K.BNSTAT_SHAPES)
@pytest.mark.parametrize("regime", K.REGIMES)
def test_dgrad_bnstat(impl, shape, regime):
    """One and two sets, each mask source, store_masked, extra_rows, the addend forms, no ya."""
    for cfg in K.PINNED_CFGS:
        for mask in K.MASKS:
            for sets in (1, 2):
                K.check_dgrad_bnstat(impl, shape, regime, cfg, sets, mask)
        K.check_dgrad_bnstat(impl, shape, regime, cfg, 2, "bits", "masked", extra_rows=3)
        K.check_dgrad_bnstat(impl, shape, regime, cfg, 1, "bits", no_ya=True)
        if shape[6] == 1:
            K.check_dgrad_bnstat(impl, shape, regime, cfg, 1, "affine", "compact")
            for sets in (1, 2):
                K.check_dgrad_bnstat(impl, shape, regime, cfg, sets, "bits", "full", store_masked=1)


def _wgrad_row(impl, shape, cfg, steps, unit=1, layouts=("krsc",)):
    for regime in K.REGIMES:
        for splits, sink in K.wgrad_variants(impl, shape, cfg, steps, unit):
            for layout in layouts if sink else (None,):
                K.check_wgrad(impl, shape, regime, cfg, splits, layout)


@pytest.mark.parametrize("shape,cfg", K.WGRAD_GENERIC)
def test_wgrad_generic(impl, shape, cfg):
    P, Q = K.out_hw(shape)
    _wgrad_row(impl, shape, cfg, shape[0] * P * Q, 64, ("krsc", "cl"))
    K.check_wgrad(impl, shape, "wide", cfg, 0, "cl", accumulate=False)


@pytest.mark.parametrize("shape,variant", K.WGRAD_3X3)
def test_wgrad_3x3(impl, shape, variant):
    p = K.plan(impl.m, "wgrad", shape, 9)
    assert p["variant"] == variant
    _wgrad_row(impl, shape, 9, p["steps"])


@pytest.mark.parametrize("shape,variant,bn,setter", K.WGRAD_1X1)
def test_wgrad_1x1(impl, shape, variant, bn, setter):
    with K.knob(impl.m, *(setter or (None, None))):
        p = K.plan(impl.m, "wgrad", shape, 10)
        assert (p["variant"], p["bn"]) == (variant, bn)
        _wgrad_row(impl, shape, 10, p["steps"])


@pytest.mark.parametrize("Kc,C", [(64, 64), (24, 8)])
def test_splitk_reduction(impl, Kc, C):
    """Split counts at the edges of both reduction loops for each of the four thread rows, with
    and without accumulate; 24 x 8 gives 48 float4, not a multiple of the block's 64."""
    for n in K.SPLITK_COUNTS:
        shape = (n, 8, 8, C, Kc, 1, 1, 0)
        assert K.plan(impl.m, "wgrad", shape, -1, splits=n)["splits"] == n
        for regime in K.REGIMES:
            K.check_wgrad(impl, shape, regime, -1, n)
            K.check_wgrad(impl, shape, regime, -1, n, "krsc")
    shape = (33, 8, 8, C, Kc, 1, 1, 0)
    got = set()
    for req in (2, 3, 4, 5, 9, 11, 17, 33):
        got.add(K.plan(impl.m, "wgrad", shape, -1, splits=req)["splits"])
        K.check_wgrad(impl, shape, "wide", -1, req)        # the same integers for every count
    assert got == {2, 3, 4, 5, 9, 11, 17, 33}


@pytest.mark.parametrize("which", ["mixed", "duplicate", "full", "empty"])
def test_deferred_reduction(impl, which):
    """splitk_reduce_multi_kernel through the test hooks: a mixed queue, a duplicate sink (early
    flush), a full queue (18 jobs: issued at 16, then goes on) and an empty one."""
    for regime in K.REGIMES:
        if which == "mixed":
            K.check_defer_mixed(impl, regime)
        elif which == "duplicate":
            K.check_defer_duplicate(impl, regime)
        elif which == "full":
            K.check_defer_full(impl, regime)
        else:
            K.check_defer_empty(impl)


def test_env_knobs_in_fresh_processes(gpu):
    """SDX_DGRAD_MERGE=0/1 and SDX_IGEMM_GLDS=0/2 are read once per process: the strided and
    ragged rows run again in one fresh child per setting, each with its own limit; the child
    asserts through conv_plan that the knob took effect. Stops at the first child that fails."""
    for name, (env, _) in K.CHILD_SETS.items():
        e = dict(os.environ, SDX_AUTOBUILD="0", PYTHONPATH=os.pathsep.join([ROOT, TESTS]), **env)
        r = subprocess.run([sys.executable, os.path.join(TESTS, "conv_checks.py"), "--child", name], env=e,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and K.CHILD_MARKER in r.stdout, (name, r.stdout[-2000:], r.stderr[-3000:])
