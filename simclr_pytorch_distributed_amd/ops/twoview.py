"""What the native two-view losses (ops/barlow.py, ops/vicreg.py) share: the supported range of
their kernels (csrc/include/loss_gemm_plan.h) and the argument check in front of the autograd node."""
from __future__ import annotations

import torch

from ..parallel import comm

MIN_D, MAX_D = 64, 8192


def supported(n: int, D: int) -> bool:
    """Shapes the native kernels take: D = 64·j in [64, 8192], at least 2 rows, n·D < 2^31."""
    return D % 64 == 0 and MIN_D <= D <= MAX_D and n >= 2 and n * D < 2 ** 31


def check_views(name: str, z1: torch.Tensor, z2: torch.Tensor) -> None:
    """Raises unless z1, z2 are fp32 GPU views ``[n][D]`` of a :func:`supported` global batch."""
    if not (z1.is_cuda and z1.dtype == torch.float32 and z2.dtype == torch.float32 and z1.shape == z2.shape
            and z1.dim() == 2):
        raise RuntimeError(f"{name} native backend needs two fp32 GPU tensors [n][D] of equal shape")
    n, D = z1.shape[0] * comm.world_size(), z1.shape[1]
    if not supported(n, D):
        raise RuntimeError(f"{name} native backend: unsupported shape N={n}, D={D} "
                           f"(D = 64·j in [{MIN_D}, {MAX_D}], N >= 2)")
