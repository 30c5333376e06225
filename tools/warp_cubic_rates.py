"""The bicubic warp (csrc/warp_cubic.hip) timed with HIP events beside the bilinear warp
(csrc/warp.hip) on the same buffers and maps, in one process.

    python tools/warp_cubic_rates.py [--shapes c2,c3] [--reps 10]

Shapes: c2 = 2000 x 1080 x 1920, c3 = 2500 x 512 x 512 (the benchmark's), or FxHxW.  The frames
are a texture seen through small rigid motions (up to 4 px and 0.002 rad, the maps of motion
correction), so every tile takes the staged path.  The C entry points are called directly into a
preallocated output; a timed window is one call (plan kernel + tile kernel) between two events,
the two warps in alternation after a warm-up of each, `reps` times.  Bytes: the stack read once
and written once (2 * 2 * F * H * W).  The output of each warp is checked once against the other
where both must agree: a frame under an integer shift.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from kcmc_amd import _lib, stages, synthetic  # noqa: E402

SHAPES = {"c2": (2000, 1080, 1920), "c3": (2500, 512, 512)}
CHUNK = 250


def rigid(rng, F, H, W, shift=4.0, angle=0.002):
    """[F, 2, 3] forward maps: rotations of up to ``angle`` rad about the image centre and
    translations of up to ``shift`` px."""
    th = rng.uniform(-angle, angle, F)
    t = rng.uniform(-shift, shift, (F, 2))
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    M = np.zeros((F, 2, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = np.cos(th), -np.sin(th), np.sin(th), np.cos(th)
    M[:, :, 2] = c - np.einsum("fij,j->fi", M[:, :, :2], c) + t
    return M


def make_stack(F, H, W, dev, seed=0):
    rng = np.random.default_rng(seed)
    gt = rigid(rng, F, H, W)
    gt[0] = [[1, 0, 3], [0, 1, -2]]  # an integer shift: both warps must agree on this frame
    base = torch.from_numpy(synthetic.make_texture((H, W), seed=seed)).to(dev)
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    for f0 in range(0, F, CHUNK):
        f1 = min(F, f0 + CHUNK)
        stages.warp_affine_u16(base.expand((f1 - f0, H, W)).contiguous(), torch.from_numpy(gt[f0:f1]).to(dev),
                               out=src[f0:f1], inverse_map=True)
    return src, gt


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(call())
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(shape, reps, dev):
    F, H, W = shape
    src, gt = make_stack(F, H, W, dev)
    out = torch.empty_like(src)
    maps = torch.from_numpy(gt).to(dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    calls = {
        "linear": lambda: L.kcmc_warp_affine_u16(ctx, ptr(src), ptr(out), ptr(maps), F, H, W, 1, 0, st),
        "cubic": lambda: L.kcmc_warp_affine_cubic_u16(ctx, ptr(src), ptr(out), ptr(maps), F, H, W, 1, 0, st),
    }
    first = {}
    for k in calls:
        for _ in range(2):
            _lib.check(calls[k]())
        first[k] = out[0].clone()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for rep in range(reps):
        for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
            ts[k].append(timed(calls[k]))
    nbytes = 2 * 2 * F * H * W
    res = {"shape": [F, H, W], "reps": reps, "bytes": nbytes,
           "integer_shift_frames_equal": bool(torch.equal(first["linear"], first["cubic"]))}
    for k, v in ts.items():
        med = float(np.median(v))
        res[k] = {"ms_median": round(med, 3), "ms_best": round(min(v), 3),
                  "ms_p90": round(float(np.percentile(v, 90)), 3), "gb_per_s": round(nbytes / med / 1e6, 1)}
    res["cubic_over_linear"] = round(res["cubic"]["ms_median"] / res["linear"]["ms_median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    shapes = [SHAPES[s] if s in SHAPES else tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    print(json.dumps({"results": [measure(s, a.reps, dev) for s in shapes]}))


if __name__ == "__main__":
    main()
