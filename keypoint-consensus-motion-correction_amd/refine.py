"""Intensity refinement of every frame's map (csrc/refine.hip).

The hot path registers frames on a few dozen keypoints, which leaves a fraction of a pixel
of jitter in every map, and frames between samples carry an interpolated map that never saw
their pixels.  This opt-in pass (VideoAligner.REFINE = "intensity") finishes with the dense
step every motion-correction tool ends on: one linearised least-squares (Gauss-Newton) step
per frame against the mean image, for gain, offset, translation and a small rotation.
Build-defined -- the reference has no such mode; the semantics are written down in
include/kcmc.h and DESIGN.md (g1) and restated in numpy in tests/test_refine_host.py.

  band_rows      the rows per band of the kernel's output the exactness bound allows
  gradient_sums  kcmc_gradient_sums_u16: seven exact integer sums per frame over a rectangle
  gram           the frame-independent normal matrix of the regressors (b, 1, gx, gy, gr)
  solve_steps    per frame (tx, ty, theta, alpha, r): the step, its rejection rules and its
                 trust region
  compose_step   the forward map of the frame corrected by that step
  refine_frames  the pass: mean image, valid region, sums, steps, re-warp of the changed
                 frames FROM THEIR SOURCE frames, and a step kept only where the frame's
                 correlation with the mean image rose

Model: with a an aligned frame and b the reference image, a(p) ~ alpha b(p - u(p)) + beta,
u(p) = (tx - theta y', ty + theta x'), (x', y') = p - c, c = (cx, cy) the rectangle's centre.
With the integer gradients gx = b(x + 1) - b(x - 1), gy = b(y + 1) - b(y - 1) (twice the
central difference) and gr = x' gy - y' gx this is linear in (alpha, beta, qx, qy, qt):
a ~ alpha b + beta + qx gx + qy gy + qt gr, with tx = -2 qx / alpha, ty = -2 qy / alpha,
theta = -2 qt / alpha.

Grayscale stacks [F, H, W] and 2 x 3 maps only.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _intensity as _in
from . import _lib
from . import fallback as _fb
from . import quality as _q
from ._intensity import Frames, Region
from .pipeline import _runs, summary_transforms
from .stages import check_interpolation, warp_affine_u16

MOTIONS = ("rigid", "translation")
_CHUNK = 256  # frames warped and measured at a time (the candidates' scratch)


def check_options(iters, motion, max_step) -> None:
    if not isinstance(iters, (int, np.integer)) or isinstance(iters, bool) or int(iters) < 1:
        raise ValueError(f"the refinement's iterations must be an integer >= 1, got {iters!r}")
    if motion not in MOTIONS:
        raise ValueError(f"the refinement's motion must be 'rigid' or 'translation', got {motion!r}")
    try:
        ok = not isinstance(max_step, bool) and math.isfinite(float(max_step)) and float(max_step) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"the refinement's largest step must be a number > 0, got {max_step!r}")


def _rect(region: Region, H: int, W: int):
    y0, y1, x0, x1 = (int(v) for v in region)
    if not (1 <= y0 < y1 <= H - 1 and 1 <= x0 < x1 <= W - 1):
        raise ValueError(f"the rectangle {(y0, y1, x0, x1)} grown by 1 must be a non-empty part of the {H} x {W} image")
    return y0, y1, x0, x1


def band_rows(H: int, W: int, region: Region) -> int:
    """The rows per band: the kernel's sums are exact while band_rows * w * max(w, h) < 2^32
    (w, h the rectangle's sides); the largest such value, capped at max(16, ceil(h / 16)) so
    that a stack of a few frames still spreads over the device (a band is one workgroup)."""
    y0, y1, x0, x1 = _rect(region, H, W)
    w, h = x1 - x0, y1 - y0
    limit = (2 ** 32 - 1) // (w * max(w, h))
    if limit < 1:
        raise ValueError(f"a rectangle of {h} x {w} pixels is too large for exact 64-bit band sums")
    return max(1, min(limit, max(16, -(-h // 16)), h))


def gradient_sums(frames: Frames, idx: Sequence[int], ref, region: Region, rows: Optional[int] = None) -> np.ndarray:
    """[len(idx), 7] Python ints (object array): (sum a, sum a^2, sum a b, sum a gx, sum a gy,
    sum x' a gy, sum y' a gx) over ``region`` = (y0, y1, x0, x1) with a = frame idx[k], b = ``ref``
    ([H, W] uint16), gx / gy twice the central differences of b and (x', y') measured from
    ((x0 + x1) // 2, (y0 + y1) // 2).  ``frames``: one device tensor or the slabs of one
    stack; ``idx``: global frame indices (any order, repeats allowed; an index outside the
    stack gives a zero row).  Each slab sums its own frames on its own device; the kernel's
    bands (``rows`` rows each, default band_rows) are added here, exactly."""
    parts = _in._slabs(frames)
    H, W = parts[0].shape[1:]
    rect = _rect(region, H, W)
    rows = band_rows(H, W, region) if rows is None else int(rows)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    n_bands = -(-(rect[1] - rect[0]) // max(rows, 1))
    out = np.zeros((len(idx), 7), object)
    for mine, o in _in.run_indexed(_lib.load().kcmc_gradient_sums_u16, parts, idx, ref, rect, (rows,), (n_bands, 7)):
        if len(mine):
            out[mine] = _add_bands(o.cpu().numpy())
    return out


def _add_bands(bands: np.ndarray) -> np.ndarray:
    """[n, n_bands, 7] int64 -> [n, 7] Python ints: the sum over the bands, which can pass
    2^63, from the sums of the values' high and low 32-bit halves."""
    lo = (bands & 0xFFFFFFFF).sum(axis=1)
    hi = (bands >> 32).sum(axis=1)
    return hi.astype(object) * (1 << 32) + lo.astype(object)


def _dot(weights, values) -> int:
    return sum(int(w) * int(v) for w, v in zip(weights, values))


def gram(ref, region: Region, motion: str = "rigid") -> np.ndarray:
    """The normal matrix of the regressors (b, 1, gx, gy, gr) over ``region`` -- (b, 1, gx, gy)
    for motion "translation" -- as exact Python ints (object array).  It depends on the
    reference image and the rectangle only.  Every row or column sum below fits int64 while
    w * max(w, h) < 2^32 (band_rows' bound); the weights x', y' are applied in Python ints."""
    if motion not in MOTIONS:
        raise ValueError(f"the refinement's motion must be 'rigid' or 'translation', got {motion!r}")
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    if ref.dtype != np.uint16 or ref.ndim != 2:
        raise ValueError("ref must be [H, W] uint16")
    H, W = ref.shape
    band_rows(H, W, region)  # the bound
    y0, y1, x0, x1 = _rect(region, H, W)
    B = ref.astype(np.int64)
    b = B[y0:y1, x0:x1]
    gx = B[y0:y1, x0 + 1:x1 + 1] - B[y0:y1, x0 - 1:x1 - 1]
    gy = B[y0 + 1:y1 + 1, x0:x1] - B[y0 - 1:y1 - 1, x0:x1]
    n = b.size
    xs = np.arange(x0, x1, dtype=np.int64) - (x0 + x1) // 2
    ys = [y - (y0 + y1) // 2 for y in range(y0, y1)]
    py = lambda v: [int(e) for e in v]  # noqa: E731
    # per row, without temporaries: the plain sums of a product, and its sums weighted by x'
    r2 = lambda u, v: py(np.einsum("ij,ij->i", u, v))  # noqa: E731
    x2 = lambda u, v: py(np.einsum("ij,ij,j->i", u, v, xs))  # noqa: E731
    r_bgx, r_gx, r_gxgx, r_gxgy = r2(b, gx), py(gx.sum(axis=1)), r2(gx, gx), r2(gx, gy)
    G = np.zeros((5, 5), object)
    G[0, :4] = [sum(r2(b, b)), sum(py(b.sum(axis=1))), sum(r_bgx), sum(r2(b, gy))]
    G[1, 1:4] = [n, sum(r_gx), sum(py(gy.sum(axis=1)))]
    G[2, 2:4] = [sum(r_gxgx), sum(r_gxgy)]
    G[3, 3] = sum(r2(gy, gy))
    if motion == "rigid":
        x_gxgy = x2(gx, gy)
        G[0, 4] = sum(x2(b, gy)) - _dot(ys, r_bgx)
        G[1, 4] = sum(py(gy @ xs)) - _dot(ys, r_gx)
        G[2, 4] = sum(x_gxgy) - _dot(ys, r_gxgx)
        G[3, 4] = sum(x2(gy, gy)) - _dot(ys, r_gxgy)
        G[4, 4] = (_dot([int(x) ** 2 for x in xs], np.einsum("ij,ij->j", gy, gy)) - 2 * _dot(ys, x_gxgy)
                   + _dot([y * y for y in ys], r_gxgx))
    k = 5 if motion == "rigid" else 4
    G = G[:k, :k]
    for i in range(k):
        for j in range(i):
            G[i, j] = G[j, i]
    return G


def solve_steps(G: np.ndarray, sums: np.ndarray, n: int, motion: str = "rigid", max_step: float = 1.0,
                corners: Optional[Sequence[Sequence[float]]] = None) -> np.ndarray:
    """[F, 5] float64 = (tx, ty, theta, alpha, r) per frame from gram's matrix and
    gradient_sums' rows over ``n`` pixels.

    The system G p = (sum a b, sum a, sum a gx, sum a gy, sum x' a gy - sum y' a gx) is solved for
    the deviation of p from (alpha, beta, q) = (1, 0, 0): the right-hand side minus G's
    first column, in exact integers, so a frame equal to the reference gives an exactly zero
    step.  float64 from there, G scaled symmetrically by powers of two to a unit diagonal.
    r is Pearson's correlation of the frame with the reference (quality.pearson).

    Rejected -- a zero step, alpha as found or NaN -- when the frame or the reference is
    constant (r is NaN), G is singular, alpha <= 0 or a value is not finite.  Otherwise the
    step is scaled as a whole by min(1, max_step / d), d the largest |u| (max norm) at
    ``corners`` ((x', y') of the rectangle's four corner pixels; required for a step)."""
    if motion not in MOTIONS:
        raise ValueError(f"the refinement's motion must be 'rigid' or 'translation', got {motion!r}")
    k = 5 if motion == "rigid" else 4
    G = np.asarray(G, object)
    if G.shape != (k, k):
        raise ValueError(f"G must be [{k}, {k}] for motion {motion!r}, got {G.shape}")
    sums = np.asarray(sums, object).reshape(-1, 7)
    F, n = len(sums), int(n)
    out = np.zeros((F, 5))
    out[:, 3] = np.nan
    stats = np.empty((F, 5), object)  # quality.pearson's rows (sum a, sum b, sum a^2, sum b^2, sum a b)
    stats[:, 0], stats[:, 2], stats[:, 4] = sums[:, 0], sums[:, 1], sums[:, 2]
    stats[:, 1], stats[:, 3] = G[0, 1], G[0, 0]
    out[:, 4] = _q.pearson(stats, n)
    if F == 0 or any(int(G[i, i]) <= 0 for i in range(k)):
        return out
    scale = np.array([2.0 ** -round(math.log2(int(G[i, i])) / 2) for i in range(k)])
    Gs = np.array([[float(int(G[i, j])) for j in range(k)] for i in range(k)]) * scale[:, None] * scale[None, :]
    rhs = np.empty((k, F))
    for f, (sa, _, sab, sagx, sagy, sxagy, syagx) in enumerate(sums):
        full = (int(sab), int(sa), int(sagx), int(sagy), int(sxagy) - int(syagx))
        rhs[:, f] = [float(full[i] - int(G[i, 0])) for i in range(k)]
    try:
        with np.errstate(all="ignore"):
            p = np.linalg.solve(Gs, rhs * scale[:, None]) * scale[:, None]
    except np.linalg.LinAlgError:
        return out
    alpha = 1.0 + p[0]
    out[:, 3] = alpha
    with np.errstate(all="ignore"):
        t = -2.0 * p[2:k] / alpha  # [2 or 3, F]
        ok =~np.isnan(out[:, 4]) & np.isfinite(p).all(axis=0) & (alpha > 0) & np.isfinite(t).all(axis=0)
        tx, ty = t[0], t[1]
        th = t[2] if k == 5 else np.zeros(F)
        ok &= (tx != 0) | (ty != 0) | (th != 0)
        if not ok.any():
            return out
        if corners is None:
            raise ValueError("solve_steps: the trust region needs the rectangle's corners")
        d = np.zeros(F)
        for xc, yc in corners:
            d = np.maximum(d, np.maximum(np.abs(tx - th * yc), np.abs(ty + th * xc)))
        ok &= np.isfinite(d)
        s = np.where(d > 0, np.minimum(1.0, float(max_step) / d), 1.0)
        for col, v in enumerate((tx, ty, th)):
            out[ok, col] = (v * s + 0.0)[ok]
    return out


def centre(region: Region):
    """(cx, cy): the integer centre the kernel measures x', y' from."""
    y0, y1, x0, x1 = region
    return (x0 + x1) // 2, (y0 + y1) // 2


def corner_offsets(region: Region):
    """(x', y') of the rectangle's four corner pixels."""
    y0, y1, x0, x1 = region
    cx, cy = centre(region)
    return [(x - cx, y - cy) for y in (y0, y1 - 1) for x in (x0, x1 - 1)]


def compose_step(M: np.ndarray, tx: float, ty: float, theta: float, c) -> np.ndarray:
    """The forward map of a frame whose registration with M is off by the found step: the
    step says aligned(U(p)) ~ ref(p) with U(p) = c + R(theta)(p - c) + (tx, ty) (exact cos and
    sin), the corrected frame is src(M^-1(U(p))), so M' = U^-1 o M, U^-1(p) = c + R(-theta)(p - c
    - t).  For theta = 0 this is fallback.compose: the translation column lowered by the shift.
    An exact rotation keeps a euclidean map euclidean."""
    M = np.array(M, dtype=np.float64, copy=True)
    if M.shape != (2, 3):
        raise ValueError(f"compose_step: M must be [2, 3], got {M.shape}")
    if float(theta) == 0.0:
        return _fb.compose(M, tx, ty)
    co, si = math.cos(float(theta)), math.sin(float(theta))
    L = np.array([[co, si], [-si, co]])
    c = np.array([float(c[0]), float(c[1])])
    out = np.empty((2, 3))
    out[:, :2] = L @ M[:, :2]
    out[:, 2] = L @ (M[:, 2] - c - np.array([float(tx), float(ty)])) + c
    return out


@dataclass
class RefineResult:
    steps: np.ndarray         # [n_images, iters, 3] float64: the applied (tx, ty, theta); 0 where rejected or reverted
    correlations: np.ndarray  # [n_images, iters + 1] float64: r before each iteration and after the last
    idxs: List[int]           # the frames whose map changed


def refine_frames(res, sources: Sequence[torch.Tensor], n_images: int, rate: int, model: str, iters: int = 2,
                  motion: str = "rigid", max_step: float = 1.0,
                  logger: Optional[logging.Logger] = None, interpolation: str = "linear") -> RefineResult:
    """The pass over one result of the hot path (``res``: a SlabResult or SplitResult whose
    aligned frames are still on their devices; ``sources``: each slab's source frames).
    Changes ``res`` in place: the changed frames' rows of the aligned stack, of ``affines``
    and of the transform summary.  ``res.skipped`` / ``res.interpolated`` stay what they are.
    ``interpolation``: the warp's ("linear" or "cubic"); the candidates are warped with it and
    the valid region is the one of its footprint."""
    check_options(iters, motion, max_step)
    taps = 4 if check_interpolation(interpolation) == "cubic" else 2
    iters = int(iters)
    parts = _in.pass_parts("intensity refinement", res)
    H, W = parts[0].shape[1:]
    n = int(n_images)
    out = RefineResult(np.zeros((n, iters, 3)), np.full((n, iters + 1), np.nan), [])
    info = logger.info if logger is not None else (lambda msg: None)
    sel = _in.sample_mask(n, rate, res.skipped)
    changed = set()
    for it in range(iters):
        try:
            ref = _q.mean_image(parts, sel)
            rect = _q.valid_region(np.asarray(res.affines)[:n], H, W, taps=taps)
            rows = band_rows(H, W, rect)
        except ValueError as e:
            info(f"intensity refinement, iteration {it + 1}: nothing refined ({e})")
            break
        n_px = (rect[1] - rect[0]) * (rect[3] - rect[2])
        sums = gradient_sums(parts, range(n), ref, rect, rows)
        st = solve_steps(gram(ref, rect, motion), sums, n_px, motion, max_step, corner_offsets(rect))
        out.correlations[:, it] = st[:, 4]
        out.correlations[:, it + 1] = st[:, 4]
        c = centre(rect)
        moved = np.flatnonzero((st[:, :3] != 0).any(axis=1))
        new_maps = {int(i): compose_step(res.affines[i], st[i, 0], st[i, 1], st[i, 2], c) for i in moved}
        kept = []
        # the candidates, warped from their source frames
        for src, dst, f0, a, b in _in.rewarp_runs(sources, parts, new_maps, _CHUNK):
            maps = torch.from_numpy(np.stack([new_maps[f0 + j] for j in range(a, b)])).to(dst.device)
            cand = warp_affine_u16(src[a:b], maps, interpolation=interpolation)
            r_new = _q.frame_correlations(cand, ref, rect)
            rose = r_new > st[f0 + a:f0 + b, 4]  # kept only there (NaN: not kept)
            for ra, rb in _runs(rose):
                dst[a + ra:a + rb].copy_(cand[ra:rb])
            idx = f0 + a + np.flatnonzero(rose)
            out.correlations[idx, it + 1] = r_new[rose]
            kept.extend(int(i) for i in idx)
        if kept:
            maps = np.stack([new_maps[i] for i in kept])
            res.affines[kept] = maps
            res.euclidean[kept] = summary_transforms(maps, model)
            out.steps[kept, it] = st[kept, :3]
        changed.update(kept)
        largest = float(np.abs(out.steps[:, it, :2]).max()) if n else 0.0
        info(f"intensity refinement, iteration {it + 1}: {len(kept)} of {n} frames stepped (largest step "
             f"{largest:.3f} px), {len(moved) - len(kept)} reverted")
    out.idxs = sorted(changed)
    return out
