"""Host-side constants of the build's ORB-style detector (csrc/orb.hip).

The reference detects keypoints with OpenCV AKAZE/BRISK (VA:22-25, VA:114-116,
VA:190-192) and BASELINE config 2 names ORB; OpenCV is absent from this image, so the
detector is build-defined.  Its tables are generated here deterministically and shared
by the HIP kernels and the CPU oracle:

* the steered-BRIEF test pattern: 256 point pairs drawn once from N(0, (31/5)^2) per
  axis, rounded, restricted to the radius-13 disc (seeded numpy Generator);
* per orientation bin k (32 bins of 2 pi / 32), the pattern rotated to the bin centre
  (k + 1/2) 2 pi / 32 and rounded half-to-even: int8 [32, 512, 2] (x, y);
* the bin edges' (cos, sin) used by the exact bin tests: f64 [32, 2].

The scale pyramid (opt-in: ``OrbParams.n_levels`` > 1) is build-defined too.  The host
computes every level size and quota here as integers; the kernels receive integers only:

* level sizes: ``H_l = rint(H / scale_factor**l)`` (half to even, Python doubles), ``W_l``
  alike; level l is the exact bilinear resize (csrc/resize.hip) of level l - 1;
* quotas: with ``f = 1 / scale_factor`` and ``d_0 = n_features (1 - f) / (1 - f**n_levels)``,
  level ``l < n_levels - 1`` gets ``rint(d_l)``, ``d_{l+1} = d_l f``; the last level gets
  ``max(n_features - sum, 0)``.  A level's unused quota is not redistributed;
* every level runs the single-level detector unchanged with its quota as the budget; a
  level smaller than ``2 edge + 1`` in either axis, or with quota 0, yields nothing;
* output rows: level 0 first, a level's candidate order inside it, packed without gaps;
  coordinates go back to level 0 through the resize's own pixel map
  (``level_to_base``), not OpenCV's ``x * scale``.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

N_BINS = 32
N_PAIRS = 256
PATTERN_RADIUS = 13


@dataclass(frozen=True)
class OrbParams:
    """Detector parameters (defaults follow cv2.ORB_create where they apply:
    nfeatures=500, fastThreshold=20, edgeThreshold=31 -> 16-pixel margin here,
    HARRIS_SCORE with k = 0.04).  n_levels = 1 (the default) is the single-scale detector;
    n_levels in 2..8 detects on a scale pyramid of ratio scale_factor (> 1) and shares
    n_features among the levels (level_sizes, level_quotas)."""

    n_features: int = 500
    fast_threshold: int = 20
    harris_k: float = 0.04
    edge: int = 16
    n_levels: int = 1
    scale_factor: float = 1.2


MAX_LEVELS = 8


def _check_pyramid(n_levels: int, scale_factor: float) -> None:
    if not 1 <= int(n_levels) <= MAX_LEVELS:
        raise ValueError(f"n_levels must be in [1, {MAX_LEVELS}]")
    if not float(scale_factor) > 1.0:
        raise ValueError("scale_factor must be > 1")


def level_sizes(H: int, W: int, n_levels: int, scale_factor: float = 1.2):
    """[(H_l, W_l)] for l in range(n_levels): rint(H / scale_factor**l), half to even."""
    _check_pyramid(n_levels, scale_factor)
    s = float(scale_factor)
    return [(int(round(H / s ** l)), int(round(W / s ** l))) for l in range(int(n_levels))]


def level_quotas(n_features: int, n_levels: int, scale_factor: float = 1.2):
    """The levels' keypoint budgets (a geometric series of ratio 1 / scale_factor, rounded
    half to even; the last level takes what is left).  They sum to n_features."""
    _check_pyramid(n_levels, scale_factor)
    n_levels, n_features = int(n_levels), int(n_features)
    f = 1.0 / float(scale_factor)
    d = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(round(d)))
        total += out[-1]
        d *= f
    out.append(max(n_features - total, 0))
    return out


def level_to_base(c, n_base: int, n_level: int):
    """A level pixel index (scalar or array) along one axis -> its level-0 coordinate, the
    resize's own pixel map: ((2 c + 1) n_base - n_level) / (2 n_level), one double division."""
    c = np.asarray(c, np.int64)
    return ((2 * c + 1) * int(n_base) - int(n_level)).astype(np.float64) / np.float64(2 * int(n_level))


@lru_cache(maxsize=4)
def brief_pattern(seed: int = 7) -> np.ndarray:
    """[512, 2] int: points 2i and 2i+1 form BRIEF pair i."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < 2 * N_PAIRS:
        x, y = np.rint(rng.normal(0.0, 31.0 / 5.0, 2))
        if x * x + y * y <= PATTERN_RADIUS * PATTERN_RADIUS:
            pts.append((int(x), int(y)))
    return np.array(pts, dtype=np.int64)


@lru_cache(maxsize=4)
def rotated_patterns(seed: int = 7) -> np.ndarray:
    p = brief_pattern(seed).astype(np.float64)
    out = np.empty((N_BINS, 2 * N_PAIRS, 2), np.int8)
    for k in range(N_BINS):
        a = (k + 0.5) * 2.0 * np.pi / N_BINS
        c, s = np.cos(a), np.sin(a)
        out[k, :, 0] = np.rint(p[:, 0] * c - p[:, 1] * s)
        out[k, :, 1] = np.rint(p[:, 0] * s + p[:, 1] * c)
    return out


@lru_cache(maxsize=1)
def bin_edges() -> np.ndarray:
    a = np.arange(N_BINS) * 2.0 * np.pi / N_BINS
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))
