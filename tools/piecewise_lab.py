"""Measurements of the piecewise-rigid mode (a record, nothing gates on it): profiles/piecewise.md.

    python tools/piecewise_lab.py [--out FILE] [--reps 7] [--inner 4]

1. warp: kcmc_warp_field_u16 against kcmc_warp_affine_u16 on the same device-resident frames
   and maps in one process, interleaved (affine, zero field, +-2 px field, repeated), at
   config 2's frame shape (1080 x 1920) and config 3's (512 x 512), grid (4, 4).  Every timed
   window is `inner` calls between two events after a warm-up of the same shape.  Both warps
   read and write the stack once, so the yardstick is the affine warp's time; the ratio is
   reported.
2. ransac: the per-cell launch (2000 frames x 16 cells, one virtual frame each) next to the
   global launch (2000 frames, 100 consensus points) -- HIP events around stages.ransac_rigid --
   and the whole of piecewise.fit_cells (host clock, synchronised).
3. accuracy: synthetic keypoints under a global rigid motion plus a known per-quadrant
   translation; RMS over frames and nodes of (true source position of the node) - (the
   position the warp uses): grid off = the global map alone, grid on = the global map plus the
   quantised field.

Prints one JSON line per part."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from kcmc_amd import piecewise, stages, synthetic  # noqa: E402

SHAPES = {"c2": (256, 1080, 1920), "c3": (2048, 512, 512)}  # frames: 1 GiB of uint16 each (beyond the L3)


def _stack(F, H, W, dev, distinct=16):
    base = synthetic.make_texture((H, W), seed=5)
    rolled = np.stack([np.roll(base, (37 * k, 53 * k), (0, 1)) for k in range(distinct)])
    # int16 view: torch repeats / copies int16 everywhere, uint16 only in places
    r16 = torch.from_numpy(np.ascontiguousarray(rolled).view(np.int16)).to(dev)
    return r16.repeat((F + distinct - 1) // distinct, 1, 1)[:F].contiguous().view(torch.uint16)


def _rigid(deg, tx, ty, H, W):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return [[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]]


def warp_part(dev, reps, inner, grid=(4, 4)):
    rows = []
    for name, (F, H, W) in SHAPES.items():
        frames = _stack(F, H, W, dev)
        out = torch.empty_like(frames)
        rng = np.random.default_rng(1)
        M = torch.from_numpy(np.array([_rigid(rng.normal(0, 0.2), rng.normal(0, 3), rng.normal(0, 3), H, W)
                                       for _ in range(F)])).to(dev)
        q0 = torch.zeros((F,) + grid + (2,), dtype=torch.int32, device=dev)
        q2 = torch.from_numpy(rng.integers(-2048, 2049, (F,) + grid + (2,)).astype(np.int32)).to(dev)
        runs = {"affine": lambda: stages.warp_affine_u16(frames, M, out=out),
                "field_zero": lambda: stages.warp_field_u16(frames, M, q0, out=out),
                "field_2px": lambda: stages.warp_field_u16(frames, M, q2, out=out)}
        ms = {k: [] for k in runs}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize(dev)
        for _ in range(reps):
            for k, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / inner)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        gb = 2 * frames.numel() * 2 / 1e9
        rows.append({"shape": name, "frames": F, "H": H, "W": W, "grid": list(grid),
                     "ms_median": med, "ms_min": {k: float(min(v)) for k, v in ms.items()},
                     "ms_max": {k: float(max(v)) for k, v in ms.items()},
                     "GBps_algorithmic": {k: gb / (v / 1e3) for k, v in med.items()},
                     "ratio_zero_over_affine": med["field_zero"] / med["affine"],
                     "ratio_2px_over_affine": med["field_2px"] / med["affine"]})
        del frames, out
        torch.cuda.empty_cache()
    return {"part": "warp", "reps": reps, "inner": inner, "rows": rows}


def _points(F, n, H, W, seed, quad_px=1.5, noise=0.2):
    """Template points; per frame a global rigid motion, a per-quadrant translation and noise.
    Returns (kp_tpl, kp_ordered [F, n, 2], true global maps, true quadrant offsets [F, 4, 2])."""
    rng = np.random.default_rng(seed)
    kp_tpl = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    quad = (kp_tpl[:, 0] >= W / 2).astype(int) + 2 * (kp_tpl[:, 1] >= H / 2).astype(int)
    kp = np.zeros((F, n, 2))
    G = np.zeros((F, 2, 3))
    off = rng.uniform(-quad_px, quad_px, (F, 4, 2))
    for f in range(F):
        G[f] = _rigid(rng.normal(0, 0.3), rng.normal(0, 3), rng.normal(0, 3), H, W)
        # the frame's point = inverse of the frame -> template map applied to the template point
        inv = piecewise.invert_affine(G[f])
        kp[f] = kp_tpl @ inv[:, :2].T + inv[:, 2] + off[f][quad] + rng.normal(0, noise, (n, 2))
    return kp_tpl, kp, G, off


def _lists(F, n, dev):
    off = (np.arange(F + 1) * n).astype(np.int32)
    idx = np.tile(np.arange(n, dtype=np.int32), F)
    return torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), off


def ransac_part(dev, reps, F=2000, n=100, H=1080, W=1920, grid=(4, 4)):
    kp_tpl, kp, _, _ = _points(F, n, H, W, seed=2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kp_o, kp_t = t(kp), t(kp_tpl)
    pt_off, pt_idx, off = _lists(F, n, dev)
    timed = {"global": [], "cells": []}
    inner = stages.ransac_rigid

    def run_global():
        return inner(kp_o.reshape(-1, 2), kp_t, pt_off, off, pt_idx=pt_idx, src_frame_stride=n)

    cell_info = {}

    def timed_cells(*a, **kw):  # the launch fit_cells makes, between two events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = inner(*a, **kw)
        e1.record()
        e1.synchronize()
        timed["cells"].append(e0.elapsed_time(e1))
        cell_info["virtual_frames"] = int(a[3].size - 1)
        cell_info["points"] = int(a[3][-1])
        return r

    G = run_global().params.cpu().numpy()
    whole = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run_global()
        e1.record()
        e1.synchronize()
        timed["global"].append(e0.elapsed_time(e1))
        stages.ransac_rigid = timed_cells
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fits = piecewise.fit_cells(kp_o, kp_t, pt_off, pt_idx, off, G, H, W, grid)
            torch.cuda.synchronize(dev)
            whole.append((time.perf_counter() - t0) * 1e3)
        finally:
            stages.ransac_rigid = inner
    return {"part": "ransac", "frames": F, "points_per_frame": n, "grid": list(grid), **cell_info,
            "global_launch_ms_median": float(np.median(timed["global"][1:])),
            "cell_launch_ms_median": float(np.median(timed["cells"][1:])),
            "fit_cells_total_ms_median": float(np.median(whole[1:])),
            "cells_fitted_share": float(fits.fitted.mean()), "reps": reps,
            "note": "launch times include the hypothesis-table check of stages.ransac_rigid (host)"}


def accuracy_part(dev, F=200, n=400, H=512, W=512):
    kp_tpl, kp, G_true, quad_off = _points(F, n, H, W, seed=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pt_off, pt_idx, off = _lists(F, n, dev)
    G = stages.ransac_rigid(t(kp).reshape(-1, 2), t(kp_tpl), pt_off, off, pt_idx=pt_idx,
                            src_frame_stride=n).params.cpu().numpy()
    inv_t, inv_g = piecewise.invert_affine(G_true), piecewise.invert_affine(G)
    rows = []
    for grid, window in (((2, 2), 1.0), ((2, 2), 0.5), ((4, 4), 1.0), ((4, 4), 0.5)):
        fits = piecewise.fit_cells(t(kp), t(kp_tpl), pt_off, pt_idx, off, G, H, W, grid, window=window)
        q = piecewise.fields_from_fits(fits, G, F, 1, H, W, grid)
        cy, cx = piecewise.node_centres(H, W, grid)
        cxx, cyy = np.meshgrid(cx, cy)
        quad = (cxx >= W / 2).astype(int) + 2 * (cyy >= H / 2).astype(int)  # [gy, gx]

        def at(inv):  # [F, gy, gx, 2]: the map applied to every node
            m = inv[:, None, None]
            return np.stack([m[..., 0, 0] * cxx + m[..., 0, 1] * cyy + m[..., 0, 2],
                             m[..., 1, 0] * cxx + m[..., 1, 1] * cyy + m[..., 1, 2]], -1)

        # a frame point is inv(G_true) p + its quadrant's offset, so that is the true source
        # position of node c; the warp uses inv(G) c (grid off) plus the field (grid on)
        truth = at(inv_t) + quad_off[:, quad]
        rows.append({"grid": list(grid), "window": window, "fitted_share": float(fits.fitted.mean()),
                     "rms_px_grid_off": float(np.sqrt(np.mean(np.sum((truth - at(inv_g)) ** 2, -1)))),
                     "rms_px_grid_on": float(np.sqrt(np.mean(np.sum((truth - at(inv_g) - q / 1024.0) ** 2, -1))))})
    return {"part": "accuracy", "frames": F, "points": n, "H": H, "W": W, "quadrant_offset_px": 1.5,
            "noise_px": 0.2, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--parts", default="warp,ransac,accuracy")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("piecewise_lab needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = []
    for p in a.parts.split(","):
        r = {"warp": lambda: warp_part(dev, a.reps, a.inner), "ransac": lambda: ransac_part(dev, a.reps),
             "accuracy": lambda: accuracy_part(dev)}[p]()
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
