"""The contrastive-loss HIP kernels (csrc/kernels/supcon.hip) against the split-precision fp64
oracle of tests/supcon_oracle.py, at the cases and within the derived bounds of
tests/supcon_checks.py (GPU). tests/test_supcon_oracle.py shows on the CPU that a correct fp32
evaluation meets the bounds with 2x room, that each deliberate defect misses them and that each
case sits on the path it is named for."""
import pytest
import torch

import supcon_checks as K

pytestmark = pytest.mark.gpu


@pytest.fixture
def impl(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    return K.ExtImpl(_ext.require(), gpu)


def _report(stats):
    for k in sorted(stats):
        print(f"{k}: largest error / bound = {stats[k]:.4f}")


@pytest.mark.parametrize("name", K.case_names())
def test_supcon_case(impl, name):
    """Forward (loss, rows, lse, invcnt), two-output backward (dA, dC) and, where the anchors are
    the contrasts, the merged backward (dX); no-positive rows and g = 0 exactly 0."""
    stats = {}
    K.check_case(impl, name, stats)
    _report(stats)


@pytest.mark.parametrize("name", K.REPEAT_CASES)
def test_supcon_repeatable(impl, name):
    """Bit-identical outputs over three calls (no atomics, fixed split order)."""
    K.check_repeat(impl, name)


def test_supcon_split_count_binding(gpu):
    from simclr_pytorch_distributed_amd.ops import _ext
    m = _ext.require()
    for a, b in [(1, 33), (65, 65), (200, 200), (129, 257), (1500, 1500), (96, 384), (384, 96), (1024, 8192)]:
        assert m.supcon_num_splits(a, b) == K.pick_splits(a, b), (a, b)


def test_supcon_autograd_wrapper(gpu):
    """ops.contrastive.supcon_rows_loss: bf16 inputs, a strided A, ``A is C`` and ``A = C * 1.0``
    inside the bounds of one oracle, gradient dtypes equal to the input dtypes."""
    stats = {}
    K.check_wrapper(gpu, stats)
    _report(stats)
