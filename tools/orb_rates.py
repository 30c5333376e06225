"""Detection (f1, csrc/orb.hip) rate at the bench's 1080p shape with an output digest, for
same-box A/B of library builds (KCMC_TEST_ONLY_ALT_LIB=1 KCMC_LIB_PATH=ab/<name>.so):

    python tools/orb_rates.py [--frames 2000] [--reps 5] [--levels 1] [--scale-factor 1.2]

--levels > 1 times the scale pyramid (kcmc_orb_detect_pyramid; the digest then covers the
level column too, and the line adds the first level's resize alone and a device copy of the
stack, ms and TB/s); --levels 1 is the single-scale entry, as before.

The stack is bench.py's c2 frames (the texture seen through each frame's jitter) scaled
to u8; stages.detect_orb is timed with HIP events around each call.  Prints one JSON
line: median / best ms, frames per second and a digest of (keypoints, descriptors,
counts), which must agree between builds."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from kcmc_amd import orb, stages  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--levels", type=int, default=1)
    ap.add_argument("--scale-factor", type=float, default=1.2)
    a = ap.parse_args()
    params = orb.OrbParams(n_levels=a.levels, scale_factor=a.scale_factor)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bc = bench.CONFIGS["c2"]
    inp, _ = bench.make_inputs(bc, a.frames, 0, dev)
    u8 = stages.max_scale_u8(inp.frames, stages.brightest_px(inp.frames))
    del inp
    k = stages.detect_orb(u8, params)
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        k = stages.detect_orb(u8, params)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    h = hashlib.sha1()
    cnt = k.count.cpu().numpy()
    h.update(cnt.tobytes())
    kp, des = k.kp.cpu().numpy(), k.des.cpu().numpy()
    for f in range(len(cnt)):
        h.update(kp[f, :cnt[f]].tobytes())
        h.update(des[f, :cnt[f]].tobytes())
    if k.level is not None:
        lvl = k.level.cpu().numpy()
        for f in range(len(cnt)):
            h.update(lvl[f, :cnt[f]].tobytes())
    med = float(np.median(ts))
    extra = {}
    if a.levels > 1:  # the first level's resize alone, next to a device copy of the same stack
        (h1, w1) = orb.level_sizes(u8.shape[1], u8.shape[2], 2, a.scale_factor)[1]
        out = torch.empty((u8.shape[0], h1, w1), dtype=torch.uint8, device=dev)
        dup = torch.empty_like(u8)
        for name, fn, nbytes in (("resize_l1", lambda: stages.resize_u8(u8, h1, w1, out=out), u8.numel() + out.numel()),
                                 ("copy", lambda: dup.copy_(u8), 2 * u8.numel())):
            fn()
            tt = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                tt.append(e0.elapsed_time(e1))
            m = float(np.median(tt))
            extra[name + "_ms"] = round(m, 3)
            extra[name + "_TB_per_s"] = round(nbytes / m / 1e9, 3)
    print(json.dumps({"lib": os.environ.get("KCMC_LIB_PATH", "in-tree"), "frames": a.frames, "levels": a.levels,
                      "ms_median": round(med, 3),
                      "ms_best": round(min(ts), 3), "frames_per_s": round(a.frames / med * 1e3, 1),
                      "mean_keypoints": float(cnt.mean()), "digest": h.hexdigest()[:16], **extra}), flush=True)


if __name__ == "__main__":
    main()
