"""fp64 numpy oracle of the Gaussian-blur augmentation stage, written from the definition of
the torchvision tensor ``gaussian_blur`` (taps w_j ~ exp(-0.5 (j/sigma)^2), j = -r..r, normalised
to sum 1; separable; reflect padding that does not repeat the edge pixel; no clamp), applied to
the colour images of ``aug_oracle.oracle_batch`` and normalised.

As in ``aug_oracle``, only the random draws come from the implementation: each view's
``(blur, sigma)`` are the two draws ``augment._view_params`` takes after the gray draw.

``EPS_BLUR_REF`` is the measured worst deviation of the fp32 torch ``augment_reference`` from
this oracle over ``CASES`` in pre-normalise colour units (tests/test_blur_oracle.py measures and
asserts it). It is set by blur_224_k23 alone, where the fp32 source coordinate of the bilinear
resize of a ~300-pixel random-noise source is off by a few 1e-5 pixels (3.5e-5 colour units
before the 23 taps average it down). Every other case stays at or below aug_oracle's EPS_REF
(blur_strips too: its 63 wide taps average the same coordinate error away), so those are held to
their own measured worst, ``EPS_BLUR_REF_REST``; ``eps_ref(name)`` is the floor of a case, from
which tests/test_gpu_blur.py derives the GPU acceptance floor.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import aug_oracle as O

# worst |augment_reference - oracle| over CASES, colour units in [0, 1] (measured; asserted in
# tests/test_blur_oracle.py::test_reference_matches_oracle)
EPS_BLUR_REF = 1.9e-5
# the same, measured over the cases other than blur_224_k23 (the worst is blur_strips, then
# blur_ragged), so that the small-radius and reflect cases are not held to the 224 case's floor
EPS_BLUR_REF_REST = 1.4e-6


def eps_ref(name: str) -> float:
    """The measured reference floor that applies to a case."""
    return EPS_BLUR_REF if name == "blur_224_k23" else EPS_BLUR_REF_REST


def reflect_index(n_out_lo: int, n_out_hi: int, n: int) -> np.ndarray:
    """Source index of the padded positions n_out_lo..n_out_hi-1 of an axis of length n:
    -j -> j and n-1+j -> n-1-j."""
    i = np.arange(n_out_lo, n_out_hi)
    i = np.where(i < 0, -i, i)
    i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    assert i.min() >= 0 and i.max() <= n - 1, "radius beyond n - 1: reflection undefined"
    return i


def weights(k: int, sigma: float) -> np.ndarray:
    assert k % 2 == 1 and k >= 3
    r = (k - 1) // 2
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * (j / float(sigma)) ** 2)
    return w / w.sum()


def gaussian_blur(c: np.ndarray, k: int, sigma: float) -> np.ndarray:
    """[S, S, 3] float64 -> [S, S, 3] float64."""
    S = c.shape[0]
    assert c.shape == (S, S, 3)
    r = (k - 1) // 2
    w = weights(k, sigma)
    src = reflect_index(-r, S + r, S)
    px = c[:, src]                                            # pad x
    c = sum(w[j] * px[:, j:j + S] for j in range(k))
    py = c[src]                                               # pad y
    return sum(w[j] * py[j:j + S] for j in range(k))


def oracle_batch(case):
    """([V*B, S, S, 3] colour, normalised) float64 with the blur applied to the rows whose
    blur draw is true."""
    cfg = case["cfg"]
    colour, _ = O.oracle_batch(case, case["rows"])
    out = np.stack([gaussian_blur(c, cfg.blur_k, r["p"]["sigma"]) if r["p"]["blur"] else c
                    for c, r in zip(colour, case["rows"])])
    return out, (out - np.asarray(cfg.mean)) / np.asarray(cfg.std)


# ---------------------------------------------------------------- cases ------------------------

def _big_ragged():
    return O._ragged([(256, 320), (313, 259)], 11)


# the seed of blur_simclr_32 was picked on the CPU so that both blur outcomes each cover >= 25 %
# of the views and fragile views are <= 5 % (tests/test_blur_oracle.py::test_case_conditions)
BLUR_SIMCLR_SEED = 3

# blur_strips: the smallest view whose ring does not fit the LDS at full width (k = 63: 64 rows
# of S pixels x 12 B pass 160 KiB from S = 214 on), at an odd S so the last strip is partial;
# sigma wide enough that the far taps, and so the whole staged halo, carry weight. Its seed was
# picked on the CPU so that neither view is fragile.
BLUR_STRIPS_SEED = 1

_BUILDERS = {
    "blur_8_k3": lambda: O._case("blur_8_k3", O._cfg(8, blur_p=1.0), 3, [3, 0, 3, 6, 0], O._dense(7, 8, 8, 1)),
    "blur_reflect_max": lambda: O._case("blur_reflect_max", O._cfg(5, blur_p=1.0, blur_kernel=9, blur_sigma=(1.5, 2.0)),
                                        4, [2, 0, 3, 1], O._dense(4, 5, 5, 2)),
    "blur_sigma_tiny": lambda: O._case("blur_sigma_tiny", O._cfg(16, blur_p=1.0, blur_kernel=7, blur_sigma=(0.1, 0.1)),
                                       5, [1, 0, 2], O._dense(3, 16, 16, 3)),
    "blur_odd_row": lambda: O._case("blur_odd_row", O._cfg(7, 3, blur_p=1.0, blur_kernel=5), 6, [2, 0, 3, 3, 1],
                                    O._dense(4, 7, 7, 4)),
    "blur_simclr_32": lambda: O._case("blur_simclr_32", O._cfg(32, blur_p=0.5, **O.SIMCLR), BLUR_SIMCLR_SEED,
                                      list(range(32)), O._dense(32, 32, 32, 6)),
    "blur_ragged": lambda: O._case("blur_ragged", O._cfg(32, blur_p=1.0, **O.SIMCLR), O.CROP_SEED,
                                   [i % 5 for i in range(20)], ragged=O._ragged(O.RAGGED_CROP, 7)),
    "blur_224_k23": lambda: O._case("blur_224_k23", O._cfg(224, 2, blur_p=1.0, **O.SIMCLR), 9, [1, 0],
                                    ragged=_big_ragged()),
    "blur_strips": lambda: O._case("blur_strips", O._cfg(215, 2, blur_p=1.0, blur_kernel=63, blur_sigma=(6.0, 10.0),
                                                         **O.SIMCLR), BLUR_STRIPS_SEED, [1], ragged=_big_ragged()),
}

CASES = list(_BUILDERS)
_cache = {}


def get_case(name):
    """Case inputs with the oracle attached (computed once per process, never modified)."""
    if name not in _cache:
        case = _BUILDERS[name]()
        case["rows"] = O.views(case)
        case["colour"], case["norm"] = oracle_batch(case)
        _cache[name] = case
    return _cache[name]


def without_blur(case):
    """The same case with the blur stage off (inputs shared, no oracle attached)."""
    off = dict(case)
    off["cfg"] = dataclasses.replace(case["cfg"], blur_p=0.0)
    for key in ("rows", "colour", "norm"):
        off.pop(key, None)
    return off
