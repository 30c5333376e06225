"""The tile gradient-sums kernel (csrc/refine_tiles.hip) timed with HIP events beside
kcmc_gradient_sums_u16 on the same buffers and rectangle, and the cost and effect of one whole
iteration of the opt-in non-rigid intensity refinement (kcmc_amd.refine_field).

    python tools/refine_field_rates.py [--frames 2000] [--grid 8] [--reps 10]
    python tools/refine_field_rates.py --pass [--frames 2000] [--grid 8] [--rounds 3]

Rates: `frames` frames of 1080 x 1920 (a texture seen through small rigid motions) against their
mean image over the valid region, tiled for a grid x grid field (2 grid x 2 grid tiles).  Both
kernels read the same bytes -- the stack once, the reference image from cache; the tile kernel
has the same four products per pixel and none of the coordinate moments, but keeps its sums per
pixel column and sorts them into tiles.  The C entry points are called directly into
preallocated outputs; a timed window is one call between two events, the two kernels in
alternation after a warm-up of each, `reps` times.  The tiles' totals must equal the first
five of kcmc_gradient_sums_u16's sums.

--pass: refine_field.refine_field_frames (one iteration: mean image, shrunk valid region, tile
sums, per-tile Gram sums and node steps on the host, the candidates' field warp from their
sources, their correlations, the copies) on a stack whose sources carry a smooth sub-pixel
field each (a linear variation over the frame of up to +-`--amp` px per component plus an
offset of a fifth of that; consecutive frames carry opposite fields, so the mean image stays
in place), with the RMS distance of the nodes' displacements from the truth before (the zero
field) and after.

Each mode prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kcmc_amd import _lib, quality, refine, refine_field, stages, synthetic  # noqa: E402
from refine_rates import H, W, make_stack, rigid, timed, warp_all  # noqa: E402


def rates(a, dev):
    F, grid = a.frames, (a.grid, a.grid)
    src, gt, _ = make_stack(F, dev)
    aligned = torch.empty_like(src)
    warp_all(src, gt, aligned)
    del src
    ref = quality.mean_image(aligned)
    rect = quality.valid_region(gt, H, W)
    rows = refine.band_rows(H, W, rect)
    n_bands = -(-(rect[1] - rect[0]) // rows)
    re, ce = refine_field.tile_edges(H, W, grid, rect)
    ty, tx = len(re) - 1, len(ce) - 1
    sums = torch.empty((F, n_bands, 7), dtype=torch.int64, device=dev)
    tiles = torch.empty((F, ty, tx, 5), dtype=torch.int64, device=dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    P = ctypes.c_void_p
    calls = {
        "tile_gradient_sums": lambda: L.kcmc_tile_gradient_sums_u16(ctx, ptr(aligned), F, H, W, None, F, ptr(ref),
                                                                    re.ctypes.data_as(P), ty, ce.ctypes.data_as(P), tx,
                                                                    ptr(tiles), st),
        "gradient_sums": lambda: L.kcmc_gradient_sums_u16(ctx, ptr(aligned), F, H, W, None, F, ptr(ref), *rect, rows,
                                                          ptr(sums), st),
    }
    ts = {k: [] for k in calls}
    for k in calls:
        for _ in range(2):
            _lib.check(calls[k]())
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
            ts[k].append(timed(calls[k]))
    n_px = (rect[1] - rect[0]) * (rect[3] - rect[2])
    res = {"shape": [F, H, W], "rect": list(rect), "grid": list(grid), "tiles": [ty, tx], "band_rows": rows,
           "n_bands": n_bands, "reps": a.reps}
    for k, v in ts.items():
        med = float(np.median(v))
        res[k] = {"ms_median": round(med, 3), "ms_best": round(min(v), 3),
                  "ms_p90": round(float(np.percentile(v, 90)), 3), "stack_gb_per_s": round(2 * F * n_px / med / 1e6, 1)}
    res["tile_over_gradient_sums"] = round(res["tile_gradient_sums"]["ms_median"] / res["gradient_sums"]["ms_median"], 3)
    res["tile_totals_equal_the_first_five_sums"] = bool(torch.equal(tiles.sum(dim=(1, 2)), sums.sum(dim=1)[:, :5]))
    return res


def smooth_fields(rng, F, grid, amp):
    """[F, gy, gx, 2] px: the node values of linear fields A p + o, p the node's position in
    [-0.5, 0.5]^2, |A| entries <= amp, |o| components <= amp / 5; frame 2k + 1 carries the negative of frame 2k's."""
    gy, gx = grid
    A = rng.uniform(-amp, amp, (F, 2, 2))
    o = rng.uniform(-amp / 5, amp / 5, (F, 2))
    py, px = np.meshgrid((np.arange(gy) + 0.5) / gy - 0.5, (np.arange(gx) + 0.5) / gx - 0.5, indexing="ij")
    u = o[:, None, None, :] + np.einsum("fab,ijb->fija", A, np.stack([px, py], -1))
    u[1::2] = -u[0:2 * (F // 2):2]
    return u


def whole_pass(a, dev):
    F, grid = a.frames, (a.grid, a.grid)
    rng = np.random.default_rng(1)
    gt = rigid(rng, F, 4.0, 0.002)
    truth = smooth_fields(rng, F, grid, a.amp)  # the correction, in aligned coordinates
    q_src = np.rint(-truth * 1024).astype(np.int32)  # what the sources carry: content(p + q)
    base = torch.from_numpy(synthetic.make_texture((H, W), seed=0)).to(dev)
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    for f0 in range(0, F, 250):
        f1 = min(F, f0 + 250)
        stages.warp_field_u16(base.expand((f1 - f0, H, W)).contiguous(), torch.from_numpy(gt[f0:f1]).to(dev),
                              torch.from_numpy(q_src[f0:f1]).to(dev), out=src[f0:f1], inverse_map=True)
    aligned = torch.empty_like(src)
    scratch = torch.empty_like(src)

    def rms(field):
        return float(np.sqrt(((field - truth) ** 2).sum(axis=-1).mean()))

    ts = {"warp": [], "field": []}
    info = {}
    for rnd in range(a.rounds + 1):  # round 0 warms up
        for mode in (list(ts) if rnd % 2 == 0 else list(ts)[::-1]):
            if mode == "field":  # the state the refinement leaves: frames warped with their maps
                warp_all(src, gt, aligned)
                res = SimpleNamespace(aligned=aligned, affines=gt.copy(), skipped=[], interpolated=[])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "warp":
                warp_all(src, gt, scratch)
            else:
                ff = refine_field.refine_field_frames(res, [src], F, 1, grid, iters=1, max_step=a.max_step)
            torch.cuda.synchronize()
            if rnd:
                ts[mode].append((time.perf_counter() - t0) * 1e3)
            if mode == "field":
                info = {"kept": len(ff.idxs), "node_error_px_rms_before": round(rms(np.zeros_like(truth)), 4),
                        "node_error_px_rms_after": round(rms(ff.field), 4),
                        "mean_r_before": round(float(np.nanmean(ff.correlations[:, 0])), 6),
                        "mean_r_after": round(float(np.nanmean(ff.correlations[:, 1])), 6)}
    w, r = float(np.median(ts["warp"])), float(np.median(ts["field"]))
    return {"shape": [F, H, W], "grid": list(grid), "amp_px": a.amp, "rounds": a.rounds,
            "warp_ms": [round(t, 1) for t in ts["warp"]], "field_ms": [round(t, 1) for t in ts["field"]],
            "warp_ms_median": round(w, 1), "field_iteration_ms_median": round(r, 1),
            "iteration_over_warp": round(r / w, 2), **info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pass", dest="whole", action="store_true")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--max-step", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    print(json.dumps(whole_pass(a, dev) if a.whole else rates(a, dev)))


if __name__ == "__main__":
    main()
