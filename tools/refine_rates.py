"""The gradient-sums kernel (csrc/refine.hip) timed with HIP events beside kcmc_frame_stats_u16
on the same buffers, and the cost of one whole iteration of the opt-in intensity refinement
beside the warp alone.

    python tools/refine_rates.py [--frames 2000] [--reps 10]
    python tools/refine_rates.py --pass [--frames 2000] [--rounds 5]

Rates: `frames` frames of 1080 x 1920 (a texture seen through small rigid motions) against their
mean image over the valid region.  Both kernels read the same bytes -- the stack once, the
reference image from cache -- and differ in arithmetic: four multiply-adds per pixel and the
row / column bookkeeping of the weighted sums against frame_stats' two.  The C entry points
are called directly into preallocated outputs; a timed window is one call between two
events, the two kernels in alternation after a warm-up of each, `reps` times.  The sums'
first three columns must equal frame_stats' (sum a, sum a^2, sum a b).

--pass: refine.refine_frames (one iteration, every frame stepped: mean image, valid region,
sums, Gram matrix and steps on the host, the candidates' warp from their sources, their
correlations, the copies) on a stack whose maps carry 0.3 - 0.5 px of jitter, in alternation
with warp_affine_u16 of the same frames alone.

--pass --parts: the same with a device synchronise and a host clock around the pass's parts
(which serialises them: the parts' shares, not a second total).

Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from kcmc_amd import _lib, quality, refine, stages, synthetic  # noqa: E402
from kcmc_amd.pipeline import summary_transforms  # noqa: E402

H, W = 1080, 1920


def rigid(rng, F, shift, angle):
    """[F, 2, 3] forward maps: rotations of up to ``angle`` rad about the image centre and
    translations of up to ``shift`` px."""
    th = rng.uniform(-angle, angle, F)
    t = rng.uniform(-shift, shift, (F, 2))
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    M = np.zeros((F, 2, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    M[:, :, 2] = c - np.einsum("fij,j->fi", M[:, :, :2], c) + t
    return M


def make_stack(F, dev, seed=0):
    """Sources whose true forward maps are ``gt``: the texture seen through their inverses."""
    rng = np.random.default_rng(seed)
    gt = rigid(rng, F, 4.0, 0.002)
    base = torch.from_numpy(synthetic.make_texture((H, W), seed=seed)).to(dev)
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    for f0 in range(0, F, 250):
        f1 = min(F, f0 + 250)
        maps = torch.from_numpy(gt[f0:f1]).to(dev)
        stages.warp_affine_u16(base.expand((f1 - f0, H, W)).contiguous(), maps, out=src[f0:f1], inverse_map=True)
    return src, gt, rng


def warp_all(src, maps_np, out):
    for f0 in range(0, len(maps_np), 250):
        f1 = min(len(maps_np), f0 + 250)
        stages.warp_affine_u16(src[f0:f1], torch.from_numpy(maps_np[f0:f1]).to(src.device), out=out[f0:f1])


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rates(a, dev):
    F = a.frames
    src, gt, _ = make_stack(F, dev)
    aligned = torch.empty_like(src)
    warp_all(src, gt, aligned)
    del src
    ref = quality.mean_image(aligned)
    rect = quality.valid_region(gt, H, W)
    rows = refine.band_rows(H, W, rect)
    n_bands = -(-(rect[1] - rect[0]) // rows)
    sums = torch.empty((F, n_bands, 7), dtype=torch.int64, device=dev)
    stats = torch.empty((F, 5), dtype=torch.int64, device=dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    calls = {
        "gradient_sums": lambda: L.kcmc_gradient_sums_u16(ctx, ptr(aligned), F, H, W, None, F, ptr(ref), *rect, rows,
                                                          ptr(sums), st),
        "frame_stats": lambda: L.kcmc_frame_stats_u16(ctx, ptr(aligned), F, H, W, ptr(ref), *rect, ptr(stats), st),
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
    res = {"shape": [F, H, W], "rect": list(rect), "band_rows": rows, "n_bands": n_bands, "reps": a.reps}
    for k, v in ts.items():
        med = float(np.median(v))
        res[k] = {"ms_median": round(med, 3), "ms_best": round(min(v), 3),
                  "ms_p90": round(float(np.percentile(v, 90)), 3), "stack_gb_per_s": round(2 * F * n_px / med / 1e6, 1)}
    res["gradient_over_frame_stats"] = round(res["gradient_sums"]["ms_median"] / res["frame_stats"]["ms_median"], 3)
    res["first_three_sums_equal_frame_stats"] = bool(torch.equal(sums.sum(dim=1)[:, :3], stats[:, [0, 2, 4]]))
    return res


PARTS = ((quality, "mean_image"), (quality, "valid_region"), (refine, "gradient_sums"), (refine, "gram"),
         (refine, "solve_steps"), (refine, "compose_step"), (refine, "warp_affine_u16"),
         (quality, "frame_correlations"))


def instrument(acc):
    """Wrap the pass's parts with synchronised host clocks that add into ``acc`` (ms)."""
    for mod, name in PARTS:
        def wrap(orig, name=name):
            def timed_part(*args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = orig(*args, **kw)
                torch.cuda.synchronize()
                acc[name] = acc.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
                return out
            return timed_part
        setattr(mod, name, wrap(getattr(mod, name)))


def whole_pass(a, dev):
    F = a.frames
    parts = {}
    if a.parts:
        instrument(parts)
    src, gt, rng = make_stack(F, dev)
    ang = rng.uniform(0, 2 * np.pi, F)
    jit = rng.uniform(0.3, 0.5, F)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    maps0 = gt.copy()
    maps0[:, :, 2] += jit
    aligned = torch.empty_like(src)
    scratch = torch.empty_like(src)

    def rms(maps):
        c = np.array([(W - 1) / 2, (H - 1) / 2, 1.0])
        d = (maps - gt) @ c
        return float(np.sqrt((d ** 2).sum(axis=1).mean()))

    ts = {"warp": [], "refine": []}
    info = {}
    for rnd in range(a.rounds + 1):  # round 0 warms up
        for mode in (list(ts) if rnd % 2 == 0 else list(ts)[::-1]):
            parts.clear()
            if mode == "refine":  # the state a hot path leaves: frames warped with the jittered maps
                warp_all(src, maps0, aligned)
                res = SimpleNamespace(aligned=aligned, affines=maps0.copy(), skipped=[], interpolated=[],
                                      euclidean=summary_transforms(maps0, "euclidean"))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "warp":
                warp_all(src, maps0, scratch)
            else:
                rf = refine.refine_frames(res, [src], F, 1, "euclidean", iters=1, motion=a.motion)
            torch.cuda.synchronize()
            if rnd:
                ts[mode].append((time.perf_counter() - t0) * 1e3)
            if mode == "refine":
                info = {"stepped": len(rf.idxs), "centre_error_px_rms_before": round(rms(maps0), 4),
                        "centre_error_px_rms_after": round(rms(res.affines), 4),
                        "mean_r_before": round(float(np.nanmean(rf.correlations[:, 0])), 6),
                        "mean_r_after": round(float(np.nanmean(rf.correlations[:, 1])), 6)}
                if a.parts:
                    info["parts_ms_last_round"] = {k: round(v, 2) for k, v in parts.items()}
    w, r = float(np.median(ts["warp"])), float(np.median(ts["refine"]))
    return {"shape": [F, H, W], "motion": a.motion, "rounds": a.rounds, "warp_ms": [round(t, 1) for t in ts["warp"]],
            "refine_ms": [round(t, 1) for t in ts["refine"]], "warp_ms_median": round(w, 1),
            "refine_iteration_ms_median": round(r, 1), "iteration_over_warp": round(r / w, 2), **info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pass", dest="whole", action="store_true")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--motion", default="rigid")
    ap.add_argument("--parts", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    print(json.dumps(whole_pass(a, dev) if a.whole else rates(a, dev)))


if __name__ == "__main__":
    main()
