"""Intensity fallback for the frames RANSAC gave no model (csrc/shift_search.hip).

The reference never registers such a frame: its map is interpolated from its neighbours
(VA:347-437) and it is warped with that guess.  This opt-in pass (VideoAligner.FALLBACK =
"correlation") registers those frames on their pixels instead.  Build-defined -- the
reference has no such mode; the semantics are written down in include/kcmc.h and
DESIGN.md (s1) and restated in numpy in tests/test_fallback_host.py.

  shift_search    kcmc_shift_search_u16: the exact correlation moments of a handful of
                  frames against a reference image at every integer shift in [-R, R]^2
  pick_shift      the peak of one frame's correlations, its rejection rules and the
                  optional parabolic sub-pixel step
  compose         the forward map of the frame corrected by that shift
  correct_skipped the pass: mean image of the registered sample frames, search over the
                  valid region shrunk by R, re-warp of the accepted frames FROM THEIR SOURCE
                  frames with the composed maps

Grayscale stacks [F, H, W] and 2 x 3 maps only.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _intensity as _in
from . import _lib
from . import quality as _q
from ._intensity import Frames, Region
from .pipeline import summary_transforms
from .stages import check_interpolation, warp_affine_u16

MAX_RADIUS = 16


def check_radius(radius) -> int:
    ok = isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) and 1 <= int(radius) <= MAX_RADIUS
    if not ok:
        raise ValueError(f"the fallback radius must be an integer in [1, {MAX_RADIUS}], got {radius!r}")
    return int(radius)


def shift_search(frames: Frames, idx: Sequence[int], ref, region: Region, radius: int) -> np.ndarray:
    """[len(idx), S, S, 5] int64, S = 2 * radius + 1: entry [k][dy + R][dx + R] = (sum a, sum b,
    sum a^2, sum b^2, sum a*b) over ``region`` = (y0, y1, x0, x1) with a = frame idx[k] read at
    (y + dy, x + dx) and b = ``ref`` ([H, W] uint16) at (y, x) -- quality.frame_stats at every
    integer shift.  ``frames``: one device tensor or the slabs of one stack; ``idx``: global
    frame indices (any order, repeats allowed; an index outside the stack gives a zero row).
    Each slab searches its own frames on its own device.  The region grown by ``radius``
    must stay inside the image."""
    parts = _in._slabs(frames)
    R = check_radius(radius)
    S = 2 * R + 1
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    out = np.zeros((len(idx), S, S, 5), np.int64)
    for rows, o in _in.run_indexed(_lib.load().kcmc_shift_search_u16, parts, idx, ref, region, (R,), (S, S, 5)):
        if len(rows):
            out[rows] = o.cpu().numpy()
    return out


class Pick(NamedTuple):
    dx: float         # the accepted shift (NaN when rejected)
    dy: float
    r_peak: float     # the largest correlation in the window (NaN when none is defined)
    accepted: bool


def pick_shift(r: np.ndarray, radius: int, min_corr: float = 0.0, subpixel: bool = True) -> Pick:
    """The shift of one frame from its [S, S] float64 correlations r[dy + R][dx + R].

    Peak: the largest r, NaN counting as -inf; ties go to the smaller dy^2 + dx^2, then the
    smaller dy, then the smaller dx.  Rejected (the frame keeps its interpolated map) when
    the peak r is NaN, is <= min_corr, or lies on the window's border (|dy| == R or
    |dx| == R: the search was saturated).  Sub-pixel (optional), per axis from the peak's two
    neighbours: den = r- - 2 r0 + r+; delta = clamp(0.5 (r- - r+) / den, -0.5, 0.5) when
    den < 0, else -- or when a neighbour is NaN -- 0."""
    R = check_radius(radius)
    S = 2 * R + 1
    r = np.asarray(r, dtype=np.float64)
    if r.shape != (S, S):
        raise ValueError(f"r must be [{S}, {S}], got {r.shape}")
    best = None
    for iy in range(S):
        for ix in range(S):
            v = r[iy, ix]
            dy, dx = iy - R, ix - R
            key = (-(-math.inf if math.isnan(v) else float(v)), dy * dy + dx * dx, dy, dx)
            if best is None or key < best:
                best = key
    _, _, dy, dx = best
    r0 = float(r[dy + R, dx + R])
    if math.isnan(r0) or r0 <= min_corr or abs(dy) == R or abs(dx) == R:
        return Pick(math.nan, math.nan, r0, False)

    def delta(lo: float, hi: float) -> float:
        if math.isnan(lo) or math.isnan(hi):
            return 0.0
        den = lo - 2.0 * r0 + hi
        if not den < 0:
            return 0.0
        return min(0.5, max(-0.5, 0.5 * (lo - hi) / den))

    sx = sy = 0.0
    if subpixel:
        sx = delta(float(r[dy + R, dx + R - 1]), float(r[dy + R, dx + R + 1]))
        sy = delta(float(r[dy + R - 1, dx + R]), float(r[dy + R + 1, dx + R]))
    return Pick(dx + sx, dy + sy, r0, True)


def compose(M: np.ndarray, dx: float, dy: float) -> np.ndarray:
    """The forward map of a frame whose registration with M is off by the found shift:
    the search says aligned(p + d) ~ ref(p), the corrected frame is src(M^-1(p + d)), so
    M' = M with the translation column lowered by d (float64, this order)."""
    out = np.array(M, dtype=np.float64, copy=True)
    if out.shape != (2, 3):
        raise ValueError(f"compose: M must be [2, 3], got {out.shape}")
    out[0, 2] = out[0, 2] - float(dx)
    out[1, 2] = out[1, 2] - float(dy)
    return out


def search_region(region: Region, radius: int) -> Optional[Region]:
    """The valid region shrunk by ``radius`` on every side; None when a side is shorter than
    2 * radius + 1."""
    y0, y1, x0, x1 = region
    y0, y1, x0, x1 = y0 + radius, y1 - radius, x0 + radius, x1 - radius
    if y1 - y0 < 2 * radius + 1 or x1 - x0 < 2 * radius + 1:
        return None
    return y0, y1, x0, x1


@dataclass
class FallbackResult:
    shifts: np.ndarray        # [len(skipped), 2] float64 (dx, dy), NaN where rejected
    correlations: np.ndarray  # [len(skipped), 2] float64 (r at zero shift, r at the peak)
    idxs: List[int]           # the frames whose map was replaced


def correct_skipped(res, sources: Sequence[torch.Tensor], n_images: int, rate: int, model: str, radius: int,
                    min_corr: float = 0.0, subpixel: bool = True,
                    logger: Optional[logging.Logger] = None, interpolation: str = "linear") -> FallbackResult:
    """The pass over one result of the hot path (``res``: a SlabResult or SplitResult whose
    aligned frames are still on their devices; ``sources``: each slab's source frames).
    Changes ``res`` in place: the accepted frames' rows of the aligned stack, of ``affines``
    and of the transform summary.  ``res.skipped`` / ``res.interpolated`` stay what they are.
    ``interpolation``: the warp's ("linear" or "cubic"); the frames are warped again with it and
    the valid region is the one of its footprint."""
    R = check_radius(radius)
    taps = 4 if check_interpolation(interpolation) == "cubic" else 2
    parts = _in.pass_parts("correlation fallback", res)
    H, W = parts[0].shape[1:]
    skipped = [int(i) for i in res.skipped if 0 <= int(i) < n_images]
    k = len(skipped)
    out = FallbackResult(np.full((k, 2), np.nan), np.full((k, 2), np.nan), [])
    if k == 0:
        return out
    info = logger.info if logger is not None else (lambda msg: None)
    try:
        ref = _q.mean_image(parts, _in.sample_mask(n_images, rate, skipped))
        rect = search_region(_q.valid_region(np.asarray(res.affines)[:n_images], H, W, taps=taps), R)
    except ValueError as e:
        info(f"correlation fallback: nothing corrected ({e})")
        return out
    if rect is None:
        info(f"correlation fallback: nothing corrected (the valid region shrunk by {R} px is narrower than "
             f"{2 * R + 1} px)")
        return out
    stats = shift_search(parts, skipped, ref, rect, R)
    S = 2 * R + 1
    r = _q.pearson(stats.reshape(-1, 5), (rect[1] - rect[0]) * (rect[3] - rect[2])).reshape(k, S, S)
    new_maps = {}
    for j, i in enumerate(skipped):
        pick = pick_shift(r[j], R, min_corr, subpixel)
        out.correlations[j] = (r[j, R, R], pick.r_peak)
        if pick.accepted:
            out.shifts[j] = (pick.dx, pick.dy)
            new_maps[i] = compose(res.affines[i], pick.dx, pick.dy)
    out.idxs = sorted(new_maps)
    # the accepted frames again, from their source frames, into their rows of the aligned stack
    for src, dst, f0, a, b in _in.rewarp_runs(sources, parts, out.idxs):
        maps = torch.from_numpy(np.stack([new_maps[f0 + j] for j in range(a, b)])).to(dst.device)
        warp_affine_u16(src[a:b], maps, out=dst[a:b], interpolation=interpolation)
    for i in out.idxs:
        res.affines[i] = new_maps[i]
        res.euclidean[i] = summary_transforms(new_maps[i][None], model)[0]
    info(f"correlation fallback: {len(out.idxs)} of {k} frames without a model registered on their pixels")
    return out
