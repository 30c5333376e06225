"""Non-rigid intensity refinement: a displacement per grid node from the pixels of every frame
(csrc/refine_tiles.hip).

The intensity refinement (kcmc_amd.refine) ends on one map per frame.  This opt-in pass
(VideoAligner.REFINE_GRID = (gy, gx) beside REFINE = "intensity") adds the patchwise step of
motion-correction tools after it: the same linearised least-squares (Gauss-Newton) step, for
gain, offset and translation, on a window around every node of a gy x gx grid, and the frame
made again by the field warp (stages.warp_field_u16) with the nodes' displacements.
Build-defined -- the reference has no such mode; the semantics are written down here, in
include/kcmc.h and DESIGN.md (g2) and restated in numpy in tests/test_refine_field_host.py.

  tile_edges          two tiles per grid cell and axis, clipped to the rectangle
  tile_gradient_sums  kcmc_tile_gradient_sums_u16: five exact integer sums per (frame, tile)
  tile_gram           the frame-independent sums per tile
  window_sums         a node's window: the sum of its (up to) 4 x 4 tiles
  solve_nodes         per (frame, node) the translation step, its rejection rules and its
                      trust region
  to_source_field     the step (aligned coordinates) as the field warp's source displacement
  refine_field_frames the pass: mean image, shrunk valid region, tile sums, node steps, the
                      candidates warped FROM THEIR SOURCE frames, kept where r rose

Tiles.  Edge k along x is clamp(k * W // (2 gx), x0, x1), k = 0 .. 2 gx, for the rectangle's
columns [x0, x1); y alike with H, gy and [y0, y1).  Cell j's two tiles are thus centred on
piecewise.node_centres' node j, the tiles cover the rectangle exactly, and a tile outside it
is empty (two equal edges).

Windows.  Node (i, j)'s window is the tile rows 2i - 1 .. 2i + 2 and the tile columns 2j - 1 ..
2j + 2, clipped to the tiling: the node's cell and half a cell to each side.  A window's sums
are the sums of its tiles' sums, in int64 (a window has fewer than 2^31 pixels).

Node step.  refine.solve_steps' system with motion "translation" on the window: regressors
(b, 1, gx, gy), normal matrix G from tile_gram's sums, right-hand side (sum a b, sum a, sum a gx,
sum a gy) minus G's first column in exact int64 (so a frame equal to the reference gives an
exactly zero step), G scaled symmetrically by the powers of two 2^-rint(log2(G_ii) / 2), one
float64 solve per node for all frames, alpha = 1 + p_0, t = -2 (p_2, p_3) / alpha.  A node gives
(0, 0) when its window is empty, a diagonal entry of G is not positive, the scaled matrix is
singular or its smallest singular value is below 1e-8 of its largest, alpha <= 0 or a value
is not finite; otherwise t is scaled by min(1, max_step / max(|tx|, |ty|)).

Field.  The step u lives in aligned coordinates (aligned(p + u) ~ ref(p)); the corrected frame
is src(M^-1 (p + u)) = src(M^-1 p + L^-1 u), L^-1 the linear part of piecewise.invert_affine(M), so
the field warp, which adds to the source coordinate, takes q = quantise(L^-1 u) (1/1024 px).

Grayscale stacks [F, H, W] and 2 x 3 maps only.
"""
from __future__ import annotations

import ctypes
import logging
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _intensity as _in
from . import _lib
from . import piecewise as _pw
from . import quality as _q
from . import refine as _rf
from ._intensity import Frames, Region
from .pipeline import _runs
from .stages import warp_field_u16

MIN_RCOND = 1e-8
_CHUNK = 256  # frames warped and measured at a time (the candidates' scratch)


def check_grid(grid) -> Tuple[int, int]:
    """(gy, gx) of a REFINE_GRID value: piecewise.check_grid's rule, two integers in [1, 16]."""
    try:
        return _pw.check_grid(grid)
    except ValueError:
        raise ValueError(f"REFINE_GRID must be None or (gy, gx) with 1 <= gy, gx <= {_pw.MAX_GRID}, "
                         f"got {grid!r}") from None


def check_iters(iters) -> int:
    if not isinstance(iters, (int, np.integer)) or isinstance(iters, bool) or int(iters) < 1:
        raise ValueError(f"REFINE_GRID_ITERS must be an integer >= 1, got {iters!r}")
    return int(iters)


def tile_edges(H: int, W: int, grid, rect: Region) -> Tuple[np.ndarray, np.ndarray]:
    """(row_edges [2 gy + 1], col_edges [2 gx + 1]) int32 of the tiling of ``rect`` = (y0, y1, x0, x1)."""
    gy, gx = grid
    y0, y1, x0, x1 = (int(v) for v in rect)
    rows = np.clip(np.arange(2 * gy + 1, dtype=np.int64) * int(H) // (2 * gy), y0, y1)
    cols = np.clip(np.arange(2 * gx + 1, dtype=np.int64) * int(W) // (2 * gx), x0, x1)
    return rows.astype(np.int32), cols.astype(np.int32)


def tile_gradient_sums(frames: Frames, idx: Sequence[int], ref, rect: Region, grid) -> np.ndarray:
    """[len(idx), 2 gy, 2 gx, 5] int64: (sum a, sum a^2, sum a b, sum a gx, sum a gy) over every tile
    of tile_edges(H, W, grid, rect), a = frame idx[k], b = ``ref`` ([H, W] uint16), gx / gy twice the
    central differences of b.  ``frames``: one device tensor or the slabs of one stack;
    ``idx``: global frame indices (any order, repeats allowed; an index outside the stack gives
    zeros).  Each slab sums its own frames on its own device."""
    parts = _in._slabs(frames)
    H, W = parts[0].shape[1:]
    rect = _rf._rect(rect, H, W)
    rows, cols = tile_edges(H, W, grid, rect)
    ty, tx = len(rows) - 1, len(cols) - 1
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    out = np.zeros((len(idx), ty, tx, 5), np.int64)
    edges = (rows.ctypes.data_as(ctypes.c_void_p), ty, cols.ctypes.data_as(ctypes.c_void_p), tx)
    for mine, o in _in.run_indexed(_lib.load().kcmc_tile_gradient_sums_u16, parts, idx, ref, (), edges, (ty, tx, 5)):
        if len(mine):
            out[mine] = o.cpu().numpy()
    return out


def tile_gram(ref, edges) -> np.ndarray:
    """[ty, tx, 10] int64: per tile of ``edges`` = (row_edges, col_edges) the sums that depend on
    the reference image only: (n, sum b, sum b^2, sum gx, sum gy, sum b gx, sum b gy, sum gx^2,
    sum gy^2, sum gx gy).  From integral images over the tiling's rectangle, exact: it has
    fewer than 2^31 pixels and every term is below 2^32 in magnitude."""
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref)
    if ref.dtype != np.uint16 or ref.ndim != 2:
        raise ValueError("ref must be [H, W] uint16")
    rows, cols = (np.asarray(e, np.int64) for e in edges)
    H, W = ref.shape
    y0, y1, x0, x1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    if (np.diff(rows) < 0).any() or (np.diff(cols) < 0).any() or y0 < 1 or y1 > H - 1 or x0 < 1 or x1 > W - 1:
        raise ValueError(f"the tiling's edges must not decrease and, grown by 1, stay inside the {H} x {W} image")
    B = ref.astype(np.int64)
    b = B[y0:y1, x0:x1]
    gx = B[y0:y1, x0 + 1:x1 + 1] - B[y0:y1, x0 - 1:x1 - 1]
    gy = B[y0 + 1:y1 + 1, x0:x1] - B[y0 - 1:y1 - 1, x0:x1]
    out = np.zeros((len(rows) - 1, len(cols) - 1, 10), np.int64)
    ru, cu = np.unique(rows) - y0, np.unique(cols) - x0  # the edges of the tiles that have pixels
    if len(ru) < 2 or len(cu) < 2:
        return out
    # tile (i, j) with pixels is segment (ri[i], ci[j]) of the distinct edges
    ri, ci = np.searchsorted(ru, rows[:-1] - y0), np.searchsorted(cu, cols[:-1] - x0)
    full = (np.diff(rows) > 0)[:, None] & (np.diff(cols) > 0)[None, :]
    pairs = ((None, None), (b, None), (b, b), (gx, None), (gy, None), (b, gx), (b, gy), (gx, gx), (gy, gy), (gx, gy))
    for k, (u, v) in enumerate(pairs):
        t = np.ones_like(b) if u is None else u if v is None else u * v
        seg = np.add.reduceat(np.add.reduceat(t, cu[:-1], axis=1), ru[:-1], axis=0)  # the last segments run to the end
        out[:, :, k] = np.where(full, seg[np.minimum(ri, len(ru) - 2)[:, None], np.minimum(ci, len(cu) - 2)[None, :]], 0)
    return out


def window_sums(tiles: np.ndarray, grid) -> np.ndarray:
    """[..., gy, gx, K] int64 from tile sums [..., 2 gy, 2 gx, K]: node (i, j) gets the tile rows
    2i - 1 .. 2i + 2 and the tile columns 2j - 1 .. 2j + 2 that exist."""
    gy, gx = grid
    tiles = np.asarray(tiles, np.int64)
    if tiles.shape[-3:-1] != (2 * gy, 2 * gx):
        raise ValueError(f"tile sums must be [..., {2 * gy}, {2 * gx}, K], got {tiles.shape}")
    out = np.zeros(tiles.shape[:-3] + (gy, gx, tiles.shape[-1]), np.int64)
    for i in range(gy):
        for j in range(gx):
            win = tiles[..., max(0, 2 * i - 1):2 * i + 3, max(0, 2 * j - 1):2 * j + 3, :]
            out[..., i, j, :] = win.sum(axis=(-3, -2))
    return out


def solve_nodes(gram_w: np.ndarray, sums_w: np.ndarray, max_step: float = 1.0) -> np.ndarray:
    """[F, gy, gx, 2] float64 px: every (frame, node)'s step (tx, ty) in aligned coordinates from
    the windows' sums (``gram_w`` [gy, gx, 10] of tile_gram's, ``sums_w`` [F, gy, gx, 5] of
    tile_gradient_sums'); (0, 0) where rejected (the module docstring has the rules)."""
    gram_w, sums_w = np.asarray(gram_w, np.int64), np.asarray(sums_w, np.int64)
    gy, gx = gram_w.shape[:2]
    if gram_w.shape != (gy, gx, 10) or sums_w.ndim != 4 or sums_w.shape[1:] != (gy, gx, 5):
        raise ValueError(f"solve_nodes: sums of [{gy}, {gx}, 10] and [F, {gy}, {gx}, 5] expected, got "
                         f"{gram_w.shape} and {sums_w.shape}")
    F = sums_w.shape[0]
    out = np.zeros((F, gy, gx, 2))
    if F == 0:
        return out
    for i in range(gy):
        for j in range(gx):
            n, sb, sbb, sgx, sgy, sbgx, sbgy, sgxx, sgyy, sgxy = gram_w[i, j]
            G = np.array([[sbb, sb, sbgx, sbgy], [sb, n, sgx, sgy], [sbgx, sgx, sgxx, sgxy], [sbgy, sgy, sgxy, sgyy]],
                         np.int64)
            if n == 0 or (np.diag(G) <= 0).any():
                continue
            scale = 2.0 ** -np.rint(np.log2(np.diag(G).astype(np.float64)) / 2)
            Gs = G.astype(np.float64) * scale[:, None] * scale[None, :]
            sa, _, sab, sagx, sagy = (sums_w[:, i, j, k] for k in range(5))
            rhs = (np.stack([sab, sa, sagx, sagy]) - G[:, :1]).astype(np.float64) * scale[:, None]  # [4, F]
            with np.errstate(all="ignore"):
                try:
                    sv = np.linalg.svd(Gs, compute_uv=False)
                    if not np.isfinite(sv).all() or not sv[0] > 0 or sv[-1] / sv[0] < MIN_RCOND:
                        continue
                    p = np.linalg.solve(Gs, rhs) * scale[:, None]
                except np.linalg.LinAlgError:
                    continue
                alpha = 1.0 + p[0]
                t = -2.0 * p[2:4] / alpha
                ok = np.isfinite(p).all(axis=0) & (alpha > 0) & np.isfinite(t).all(axis=0)
                m = np.maximum(np.abs(t[0]), np.abs(t[1]))
                s = np.where(m > 0, np.minimum(1.0, float(max_step) / np.where(m > 0, m, 1.0)), 1.0)
                out[ok, i, j, 0] = (t[0] * s + 0.0)[ok]
                out[ok, i, j, 1] = (t[1] * s + 0.0)[ok]
    return out


def to_source_field(u: np.ndarray, M: np.ndarray) -> np.ndarray:
    """q [F, gy, gx, 2] int32 (1/1024 px): the steps ``u`` [F, gy, gx, 2] (aligned coordinates) of
    frames with the forward maps ``M`` [F, 2, 3] as source displacements, quantise(L^-1 u)."""
    u = np.asarray(u, np.float64)
    inv = _pw.invert_affine(np.asarray(M, np.float64))
    a = inv[:, None, None, :, :]
    ux, uy = u[..., 0], u[..., 1]
    with np.errstate(all="ignore"):
        q = np.stack([a[..., 0, 0] * ux + a[..., 0, 1] * uy, a[..., 1, 0] * ux + a[..., 1, 1] * uy], -1)
    return _pw.quantise(np.where(np.isfinite(q), q, 0.0))


def shrunk_region(affines: np.ndarray, H: int, W: int, iters: int, max_step: float) -> Region:
    """quality.valid_region shrunk on every side by ceil(iters * max_step): no field the pass
    can keep (at most max_step per node and iteration) pulls pixels from outside the source
    into it.  ValueError when nothing is left."""
    y0, y1, x0, x1 = _q.valid_region(affines, H, W)
    m = int(math.ceil(int(iters) * float(max_step)))
    y0, y1, x0, x1 = y0 + m, y1 - m, x0 + m, x1 - m
    if y0 >= y1 or x0 >= x1:
        raise ValueError("no common valid region")
    return y0, y1, x0, x1


def correlations_from_tiles(sums: np.ndarray, gram: np.ndarray) -> np.ndarray:
    """[F] float64: every frame's Pearson correlation with the reference over the whole tiling
    (quality.pearson of the tiles' totals: what quality.frame_correlations gives there)."""
    tot = np.asarray(sums, np.int64).sum(axis=(1, 2))
    g = np.asarray(gram, np.int64).sum(axis=(0, 1))
    stats = np.empty((len(tot), 5), object)
    stats[:, 0], stats[:, 2], stats[:, 4] = tot[:, 0], tot[:, 1], tot[:, 2]
    stats[:, 1], stats[:, 3] = int(g[1]), int(g[2])
    return _q.pearson(stats, int(g[0]))


@dataclass
class FieldResult:
    field: np.ndarray         # [n_images, gy, gx, 2] float64 px, aligned coordinates: the sum of the kept steps
    correlations: np.ndarray  # [n_images, iters + 1] float64: r before each iteration and after the last
    idxs: List[int]           # the frames that kept a field


def refine_field_frames(res, sources: Sequence[torch.Tensor], n_images: int, rate: int, grid, iters: int = 1,
                        max_step: float = 1.0, logger: Optional[logging.Logger] = None) -> FieldResult:
    """The pass over one result of the hot path after refine.refine_frames (``res``: a SlabResult
    or SplitResult whose aligned frames are still on their devices; ``sources``: each slab's
    source frames).  Changes the kept frames' rows of the aligned stack in place and nothing
    else of ``res``: the maps, the transform summary, ``skipped`` and ``interpolated`` stay."""
    gy, gx = check_grid(grid)
    iters = check_iters(iters)
    parts = _in.pass_parts("intensity field refinement", res)
    H, W = parts[0].shape[1:]
    if gy > H or gx > W:
        raise ValueError(f"REFINE_GRID {(gy, gx)!r} has more nodes than the frame ({H} x {W}) has pixels")
    n = int(n_images)
    out = FieldResult(np.zeros((n, gy, gx, 2)), np.full((n, iters + 1), np.nan), [])
    info = logger.info if logger is not None else (lambda msg: None)
    sel = _in.sample_mask(n, rate, res.skipped)
    maps = np.ascontiguousarray(np.asarray(res.affines)[:n], np.float64)
    q_acc = np.zeros((n, gy, gx, 2), np.int32)  # the field every frame's pixels were made with
    changed = set()
    for it in range(iters):
        try:
            ref = _q.mean_image(parts, sel)
            rect = shrunk_region(maps, H, W, iters, max_step)
        except ValueError as e:
            info(f"intensity field refinement, iteration {it + 1}: nothing refined ({e})")
            break
        sums = tile_gradient_sums(parts, range(n), ref, rect, (gy, gx))
        gram = tile_gram(ref, tile_edges(H, W, (gy, gx), rect))
        r_old = correlations_from_tiles(sums, gram)
        out.correlations[:, it] = out.correlations[:, it + 1] = r_old
        u = solve_nodes(window_sums(gram, (gy, gx)), window_sums(sums, (gy, gx)), max_step)
        moved = np.flatnonzero((u != 0).any(axis=(1, 2, 3)))
        q_new = q_acc + to_source_field(u, maps)
        kept = []
        # the candidates, warped from their source frames
        for src, dst, f0, a, b in _in.rewarp_runs(sources, parts, moved, _CHUNK):
            g = slice(f0 + a, f0 + b)
            cand = warp_field_u16(src[a:b], torch.from_numpy(maps[g]).to(dst.device),
                                  torch.from_numpy(np.ascontiguousarray(q_new[g])).to(dst.device))
            r_new = _q.frame_correlations(cand, ref, rect)
            rose = r_new > r_old[g]  # kept only there (NaN: not kept)
            for ra, rb in _runs(rose):
                dst[a + ra:a + rb].copy_(cand[ra:rb])
            idx = f0 + a + np.flatnonzero(rose)
            out.correlations[idx, it + 1] = r_new[rose]
            kept.extend(int(i) for i in idx)
        if kept:
            q_acc[kept] = q_new[kept]
            out.field[kept] += u[kept]
        changed.update(kept)
        largest = float(np.abs(u[kept]).max()) if kept else 0.0
        info(f"intensity field refinement, iteration {it + 1}: {len(kept)} of {n} frames kept a {gy} x {gx} field "
             f"(largest node step {largest:.3f} px), {len(moved) - len(kept)} reverted")
    out.idxs = sorted(changed)
    return out
