"""Piecewise-rigid ("non-rigid") correction: per-cell rigid RANSAC and the field the field warp
(stages.warp_field_u16, csrc/warp_field.hip) interpolates.

The reference (VideoAligner.py) fits one global transform per frame and has nothing like this:
the semantics here are build-defined (DESIGN.md "Piecewise-rigid correction", include/kcmc.h)
and pinned by numpy restatements in tests/test_piecewise_host.py, not by a golden.

A gy x gx grid of nodes covers the frame.  Every sample frame that got a global model of its
own fits one rigid model per cell from the consensus points whose template keypoint lies in
the cell's window (kcmc_ransac_rigid over "virtual frames", one per (frame, cell)); the
residual of an accepted cell model against the global map, evaluated at the node, is the
node's displacement.  Frames without a model of their own (skipped frames, the non-sample
frames of a temporally downsampled stack) interpolate every entry linearly over the frame
index.  The field is quantised to 1/1024 px and the warp adds its bilinear interpolation to
the affine source coordinate.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import stages

MAX_GRID = 16


def check_grid(grid, H: Optional[int] = None, W: Optional[int] = None) -> Tuple[int, int]:
    """(gy, gx) of a PIECEWISE_GRID value; ValueError unless it is two integers in [1, 16]
    (and, with the frame size known, gy <= H and gx <= W)."""
    try:
        gy, gx = grid
        ok = int(gy) == gy and int(gx) == gx and not isinstance(gy, bool) and not isinstance(gx, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= gy <= MAX_GRID and 1 <= gx <= MAX_GRID):
        raise ValueError(f"PIECEWISE_GRID must be None or (gy, gx) with 1 <= gy, gx <= {MAX_GRID}, got {grid!r}")
    gy, gx = int(gy), int(gx)
    if (H is not None and gy > H) or (W is not None and gx > W):
        raise ValueError(f"PIECEWISE_GRID {grid!r} has more nodes than the frame ({H} x {W}) has pixels")
    return gy, gx


def check_options(min_points, window, max_residual) -> None:
    if int(min_points) != min_points or min_points < 3:
        raise ValueError("PIECEWISE_MIN_POINTS must be an integer >= 3")
    if not window > 0:
        raise ValueError("PIECEWISE_WINDOW must be > 0")
    if not max_residual >= 0:
        raise ValueError("PIECEWISE_MAX_RESIDUAL must be >= 0")


def node_centres(H: int, W: int, grid) -> Tuple[np.ndarray, np.ndarray]:
    """(cy [gy], cx [gx]) f64: node (i, j) sits at the full-resolution pixel-index coordinates
    cx_j = (j + 0.5) * W / gx - 0.5, cy_i = (i + 0.5) * H / gy - 0.5 (left to right)."""
    gy, gx = grid
    cy = (np.arange(gy, dtype=np.float64) + 0.5) * np.float64(H) / np.float64(gy) - 0.5
    cx = (np.arange(gx, dtype=np.float64) + 0.5) * np.float64(W) / np.float64(gx) - 0.5
    return cy, cx


def cell_membership(kp_full: np.ndarray, H: int, W: int, grid, window: float = 1.0) -> np.ndarray:
    """bool [gy * gx, n]: keypoint k (kp_full [n, 2] = template keypoints (x, y) scaled to full
    resolution) belongs to cell (i, j) iff |x - cx_j| <= window * W / gx and
    |y - cy_i| <= window * H / gy (fp64, inclusive)."""
    gy, gx = grid
    cy, cx = node_centres(H, W, grid)
    kp = np.asarray(kp_full, np.float64).reshape(-1, 2)
    hx = np.float64(window) * np.float64(W) / np.float64(gx)
    hy = np.float64(window) * np.float64(H) / np.float64(gy)
    in_x = np.abs(kp[None, :, 0] - cx[:, None]) <= hx  # [gx, n]
    in_y = np.abs(kp[None, :, 1] - cy[:, None]) <= hy  # [gy, n]
    return (in_y[:, None, :] & in_x[None, :, :]).reshape(gy * gx, kp.shape[0])


def accept_fit(n, n_inliers, has_model) -> np.ndarray:
    """A cell fit on n points is accepted iff it returned a model and
    n_inliers >= max(3, (n + 1) // 2)."""
    n = np.asarray(n, np.int64)
    return np.asarray(has_model, bool) & (np.asarray(n_inliers, np.int64) >= np.maximum(3, (n + 1) // 2))


def invert_affine(M: np.ndarray) -> np.ndarray:
    """OpenCV warpAffine's inversion of [..., 2, 3] maps, operation by operation (as
    oracle.invert_affine and the warps' invert_affine)."""
    M = np.asarray(M, np.float64)
    m0, m1, m2, m3, m4, m5 = (M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 0], M[..., 1, 1], M[..., 1, 2])
    with np.errstate(all="ignore"):
        D = m0 * m4 - m1 * m3
        D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
        a0, a4 = m4 * D, m0 * D
        a1, a3 = m1 * (-D), m3 * (-D)
        b1 = (-a0) * m2 - a1 * m5
        b2 = (-a3) * m2 - a4 * m5
    return np.stack([np.stack([a0, a1, b1], -1), np.stack([a3, a4, b2], -1)], -2)


def _apply(Minv: np.ndarray, cx: np.ndarray, cy: np.ndarray) -> np.ndarray:
    """[..., 2]: (M0 cx + M1 cy + M2, M3 cx + M4 cy + M5), each left to right in fp64."""
    with np.errstate(all="ignore"):
        x = Minv[..., 0, 0] * cx + Minv[..., 0, 1] * cy + Minv[..., 0, 2]
        y = Minv[..., 1, 0] * cx + Minv[..., 1, 1] * cy + Minv[..., 1, 2]
    return np.stack([x, y], -1)


def residual_field(cell_params: np.ndarray, fitted: np.ndarray, G: np.ndarray, H: int, W: int, grid,
                   max_residual: float = 8.0) -> np.ndarray:
    """r [..., gy, gx, 2] px: at node c = (cx_j, cy_i), r = inv(A_cell) c - inv(G) c for the
    cells with an accepted model (cell_params [..., gy, gx, 2, 3], fitted [..., gy, gx]; G
    [..., 2, 3] the frame's global map); 0 where there is no accepted fit, where r is not
    finite or where max(|rx|, |ry|) > max_residual (the node then follows the global model)."""
    cy, cx = node_centres(H, W, grid)
    cxx, cyy = np.meshgrid(cx, cy)  # [gy, gx]
    G = np.asarray(G, np.float64)
    r = _apply(invert_affine(cell_params), cxx, cyy) - _apply(invert_affine(G)[..., None, None, :, :], cxx, cyy)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(r).all(-1) | ~(np.abs(r).max(-1) <= np.float64(max_residual)) | ~np.asarray(fitted, bool)
    return np.where(bad[..., None], 0.0, r)


def interpolate_fields(r: np.ndarray, have: np.ndarray) -> np.ndarray:
    """Every entry of r [F, ...] interpolated linearly over the frame index between the nearest
    frames with have[f] (np.interp per entry; the nearest value held at both ends).  All zero
    when no frame has one."""
    r = np.asarray(r, np.float64)
    have = np.asarray(have, bool)
    out = np.zeros_like(r)
    xs = np.flatnonzero(have)
    if xs.size == 0:
        return out
    x = np.arange(r.shape[0])
    flat, oflat = r.reshape(r.shape[0], -1), out.reshape(r.shape[0], -1)
    for e in range(flat.shape[1]):
        oflat[:, e] = np.interp(x, xs, flat[xs, e])
    return out


def quantise(r: np.ndarray) -> np.ndarray:
    """q = int32(rint(r * 1024)): 1/1024 px, round half to even."""
    return np.rint(np.asarray(r, np.float64) * 1024).astype(np.int32)


@dataclass
class CellFits:
    """The per-cell fits of the sample frames (host arrays)."""

    points: np.ndarray      # [S, gy, gx] i32  consensus points in the cell's window
    fitted: np.ndarray      # [S, gy, gx] bool a fit was accepted, or the global model taken over
    params: np.ndarray      # [S, gy, gx, 2, 3] f64 the cell's model (NaN where not fitted)
    n_inliers: np.ndarray   # [S, gy, gx] i32  inliers of the cells that ran RANSAC (-1 elsewhere)
    ran: np.ndarray         # [S, gy, gx] bool cells that ran RANSAC


def fit_cells(kp_ordered: torch.Tensor, kp_tpl: torch.Tensor, pt_off_dev: torch.Tensor, pt_idx_dev: torch.Tensor,
              pt_off_host: np.ndarray, params_global: np.ndarray, H: int, W: int, grid, *, window: float = 1.0,
              min_points: int = 6, trials: int = 1000, residual_threshold: float = 2.0, seed: int = 42,
              spatial_rate: float = 1.0) -> CellFits:
    """The per-cell rigid fits of every sample frame, on the device of the slab.

    kp_ordered [S, n_tpl, 2] (kcmc_match_frames' ordered frame keypoints), kp_tpl [n_tpl, 2],
    the frames' consensus lists as CSR (pt_off / pt_idx: template indices in RANSAC order),
    params_global [S, 2, 3] the frames' global models (NaN: none; such a frame runs no cell
    fit -- its field is interpolated from its neighbours).  A frame's cell list keeps the order
    of the frame's list; a cell with fewer than min_points points has no fit; a cell whose
    list is the frame's whole list takes the global model; every other cell is one virtual
    frame of a single kcmc_ransac_rigid launch (pt_idx == NULL mode)."""
    gy, gx = grid
    cells = gy * gx
    dev = kp_tpl.device
    S, n_tpl = kp_ordered.shape[:2]
    ns = np.diff(np.asarray(pt_off_host)).astype(np.int64)
    G = np.asarray(params_global, np.float64).reshape(S, 2, 3)
    own = ~np.isnan(G.reshape(S, 6)).any(1)
    out = CellFits(np.zeros((S, gy, gx), np.int32), np.zeros((S, gy, gx), bool),
                   np.full((S, gy, gx, 2, 3), np.nan), np.full((S, gy, gx), -1, np.int32),
                   np.zeros((S, gy, gx), bool))
    max_n = int(ns.max()) if S else 0
    if S == 0 or max_n == 0:
        return out
    kp_full = kp_tpl.cpu().numpy() * np.float64(spatial_rate)
    member = torch.from_numpy(cell_membership(kp_full, H, W, grid, window)).to(dev)  # [cells, n_tpl]
    # the frames' lists padded to [S, max_n], then the membership mask [S, cells, max_n]
    k = torch.arange(max_n, device=dev)[None, :]
    n_dev = torch.from_numpy(ns).to(dev)[:, None]
    valid = k < n_dev
    pos = (pt_off_dev[:-1, None].long() + k).clamp_(max=max(int(pt_idx_dev.numel()) - 1, 0))
    qpad = torch.where(valid, pt_idx_dev.long()[pos], torch.zeros_like(pos))
    mask = member[:, qpad].permute(1, 0, 2) & valid[:, None, :]
    counts = mask.sum(-1).cpu().numpy().astype(np.int64)  # [S, cells]
    whole = (counts == ns[:, None]) & (counts >= min_points) & own[:, None]
    run = (counts >= min_points) & ~(counts == ns[:, None]) & own[:, None]
    out.points[:] = counts.reshape(S, gy, gx)
    out.ran[:] = run.reshape(S, gy, gx)
    P = out.params.reshape(S, cells, 2, 3)
    fitted = whole.copy()
    P[whole] = np.broadcast_to(G[:, None], (S, cells, 2, 3))[whole]
    if run.any():
        # nonzero yields (frame, cell, list position) in that order: the virtual frames' CSR
        f_i, c_i, k_i = (mask & torch.from_numpy(run).to(dev)[:, :, None]).nonzero(as_tuple=True)
        q_i = qpad[f_i, k_i]
        src = kp_ordered.reshape(S * n_tpl, 2)[f_i * n_tpl + q_i].contiguous()
        dst = kp_tpl[q_i].contiguous()
        n_v = counts[run]
        off = np.zeros(n_v.size + 1, np.int32)
        off[1:] = np.cumsum(n_v)
        rr = stages.ransac_rigid(src, dst, torch.from_numpy(off).to(dev), off, trials=trials,
                                 residual_threshold=residual_threshold, spatial_rate=spatial_rate, n_skip=3, seed=seed)
        p_v = rr.params.cpu().numpy()
        ni_v = rr.n_inliers.cpu().numpy()
        ok = accept_fit(n_v, ni_v, np.isfinite(p_v.reshape(-1, 6)).all(1))
        p_v[~ok] = np.nan
        P[run] = p_v
        out.n_inliers.reshape(S, cells)[run] = ni_v
        fitted[run] = ok
    out.fitted[:] = fitted.reshape(S, gy, gx)
    return out


def fields_from_fits(fits: CellFits, params_global: np.ndarray, n_frames: int, rate: int, H: int, W: int, grid,
                     max_residual: float = 8.0) -> np.ndarray:
    """q [n_frames, gy, gx, 2] i32: the sample frames' residual fields at their full-rate index
    (f * rate), every other frame (and every sample frame without a global model) interpolated
    over the frame index, quantised."""
    gy, gx = grid
    S = fits.points.shape[0]
    G = np.asarray(params_global, np.float64).reshape(S, 2, 3)
    own = ~np.isnan(G.reshape(S, 6)).any(1)
    n_all = max(int(n_frames), S * int(rate))
    r = np.zeros((n_all, gy, gx, 2))
    have = np.zeros(n_all, bool)
    if own.any():
        r[np.flatnonzero(own) * int(rate)] = residual_field(fits.params[own], fits.fitted[own], G[own], H, W, grid,
                                                            max_residual)
        have[np.flatnonzero(own) * int(rate)] = True
    return quantise(interpolate_fields(r, have)[:n_frames])
