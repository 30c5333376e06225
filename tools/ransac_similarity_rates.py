"""The RANSAC entry points alone, timed with HIP events at config 2's shape (2000 frames,
about 90 points each, 1000 trials): similarity (K2s) against rigid on the same points in
one process, alternating, and -- for same-box A/B of library builds -- the rigid entry of
another build (KCMC_TEST_ONLY_ALT_LIB=1 KCMC_LIB_PATH=ab/<name>.so, see tools/ab_build.py;
a build without the similarity entry times the rigid one only).

    python tools/ransac_similarity_rates.py [--frames 2000] [--points 90] [--reps 20] [--inner 200]

The points are seeded synthetic correspondences (similarity motion with a scale within 1 %
of 1, 0.3 px noise, 20 % outliers), so no matcher runs.  The C entry points are called
directly into preallocated outputs (the Python wrappers' per-call host work would otherwise
fill a window of 0.1 ms launches).  Every timed window is `inner` calls between two events
after a warm-up of the same shape; prints one JSON line with the median and best per-call
ms of each entry, their ratio and a digest of the outputs."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from kcmc_amd import _lib, stages  # noqa: E402


def make_points(frames, points, seed=3):
    rng = np.random.default_rng(seed)
    tpls, qs = [], []
    for _ in range(frames):
        n = int(rng.integers(points - 10, points + 11))
        tpl = np.stack([rng.uniform(0, 1920, n), rng.uniform(0, 1080, n)], 1)
        th, s = np.deg2rad(rng.normal(0, 0.5)), 1.0 + rng.uniform(-0.01, 0.01)
        R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        q = (tpl - rng.normal(0, 4.0, 2)) @ np.linalg.inv(R).T + rng.normal(0, 0.3, (n, 2))
        out = rng.random(n) < 0.2
        q[out] = np.stack([rng.uniform(0, 1920, int(out.sum())), rng.uniform(0, 1080, int(out.sum()))], 1)
        tpls.append(tpl.astype(np.float32).astype(np.float64))
        qs.append(q.astype(np.float32).astype(np.float64))
    off = np.zeros(frames + 1, np.int32)
    off[1:] = np.cumsum([len(q) for q in qs])
    return np.concatenate(tpls), np.concatenate(qs), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--points", type=int, default=90)
    ap.add_argument("--trials", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    tpl, q, off = make_points(a.frames, a.points)
    src, dst, off_d = (torch.from_numpy(x).to(dev) for x in (q, tpl, off))
    L = _lib.load()
    names = {"rigid": "kcmc_ransac_rigid"}
    if hasattr(L, "kcmc_ransac_similarity"):
        names["similarity"] = "kcmc_ransac_similarity"
    F, max_n = a.frames, int(np.diff(off).max())
    stages.ransac_rigid(src, dst, off_d, off, trials=a.trials)  # uploads the hypothesis tables
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    last = {k: stages.RansacResult(torch.empty((F, 2, 3), dtype=torch.float64, device=dev),
                                   torch.empty(int(off[-1]), dtype=torch.uint8, device=dev),
                                   torch.empty(F, dtype=torch.int32, device=dev),
                                   torch.empty(F, dtype=torch.int32, device=dev)) for k in names}

    def call(k):
        r = last[k]
        _lib.check(getattr(L, names[k])(ctx, ptr(src), ptr(dst), None, ptr(off_d), 0, F, max_n, a.trials, 2.0, 1.0, 3,
                                        ptr(r.params), ptr(r.inliers), ptr(r.n_inliers), ptr(r.best_trial), st))

    ts = {k: [] for k in names}
    for k in names:  # warm-up: code objects
        for _ in range(3):
            call(k)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k in names:  # alternating, so drift hits both alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                call(k)
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / a.inner)
    out = {"lib": os.environ.get("KCMC_LIB_PATH", "in-tree"), "frames": a.frames,
           "mean_points": float(np.diff(off).mean()), "trials": a.trials, "reps": a.reps, "inner": a.inner}
    for k, r in last.items():
        h = hashlib.sha1()
        for t in (r.params, r.inliers, r.n_inliers, r.best_trial):
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
        out[k] = {"ms_median": round(float(np.median(ts[k])), 4), "ms_best": round(min(ts[k]), 4),
                  "ms_p90": round(float(np.percentile(ts[k], 90)), 4),
                  "frames_fitted": int((~torch.isnan(r.params[:, 0, 0])).sum()), "digest": h.hexdigest()[:16]}
    if "similarity" in out:
        out["similarity_over_rigid"] = round(out["similarity"]["ms_median"] / out["rigid"]["ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
