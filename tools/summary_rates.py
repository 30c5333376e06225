"""The summary-image kernel (csrc/temporal_sums.hip) timed with HIP events beside the two
nearest existing reductions, the host finishing of its planes, and one data point of the
crispness of a registration under the two interpolations.

    python tools/summary_rates.py [--shapes c2,c3] [--reps 10] [--inner 5]
    python tools/summary_rates.py --finish [--size 1080x1920]
    python tools/summary_rates.py --crispness [--frames 41] [--noise 3000]

Rates: kcmc_temporal_sums_u16 with 4 and with 8 neighbours, kcmc_stack_sum_u16 (the same
bytes: the HBM floor of one read of the stack) and kcmc_gradient_sums_u16 (the nearest
kernel in arithmetic: seven 64-bit sums per pixel) on the same device-resident stack in one
process, alternating, at config 2's shape (2000 x 1080 x 1920) and config 3's
(16000 x 512 x 512).  The C entry points are called directly into preallocated outputs;
every timed window is `inner` calls between two events after a warm-up of the same shape.
Bytes are what the algorithm needs: one read of the rectangle of the selected frames (the
stack sum: of the whole stack).  The planes of the last call are checked against torch on a
few columns.

--finish: the host finishing (mean, std, correlation image, crispness) of planes of the given
size with 8 neighbours, host clock; the planes come from a small random stack on the device.

--crispness: crops of one scene at known sub-pixel shifts with independent noise, registered
with WARP_INTERPOLATION "linear" and "cubic": the crispness and the mean local correlation
of each run.  One stack; the figures depend on the data (a record, not a test).

Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kcmc_amd import VideoAligner, _lib, refine, stages, summary  # noqa: E402
from quality_rates import SHAPES, make_stack  # noqa: E402


def rates(shape_name, reps, inner, dev):
    F, H, W = SHAPES[shape_name]
    stack = make_stack(F, H, W, dev)
    ref = stack.view(torch.int16)[0].clone().view(torch.uint16)
    m = 6  # the rectangle a pass with shifts of up to 4 px would use, and one more: odd x0
    region = (m, H - m, m + 1, W - m)
    rows = refine.band_rows(H, W, region)
    n_bands = -(-(region[1] - region[0]) // rows)
    planes = torch.empty((6, H, W), dtype=torch.int64, device=dev)
    top = torch.empty((H, W), dtype=torch.uint16, device=dev)
    sums = torch.empty(H * W, dtype=torch.int64, device=dev)
    grads = torch.empty((F, n_bands, 7), dtype=torch.int64, device=dev)
    sel = torch.from_numpy((np.arange(F) % 2 == 0).view(np.uint8)).to(dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr

    def temporal(nb, s=None):
        return lambda: L.kcmc_temporal_sums_u16(ctx, ptr(stack), F, H, W, ptr(s), *region, nb, ptr(planes), ptr(top),
                                                st)

    calls = {
        "stack_sum": lambda: L.kcmc_stack_sum_u16(ctx, ptr(stack), F, H * W, None, ptr(sums), st),
        "temporal_sums_4": temporal(4),
        "temporal_sums_8": temporal(8),
        "temporal_sums_8_half": temporal(8, sel),
        "gradient_sums": lambda: L.kcmc_gradient_sums_u16(ctx, ptr(stack), F, H, W, None, F, ptr(ref), *region, rows,
                                                          ptr(grads), st),
    }
    rect_bytes = 2 * F * (region[1] - region[0]) * (region[3] - region[2])
    nbytes = {"stack_sum": 2 * F * H * W, "temporal_sums_4": rect_bytes, "temporal_sums_8": rect_bytes,
              "temporal_sums_8_half": rect_bytes // 2, "gradient_sums": rect_bytes}
    ts = {k: [] for k in calls}
    for k, c in calls.items():  # warm-up: code objects
        for _ in range(2):
            _lib.check(c())
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, c in calls.items():  # alternating, so drift hits all alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                _lib.check(c())
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    res = {"shape": [F, H, W], "region": list(region), "band_rows": rows}
    for k in calls:
        med = float(np.median(ts[k]))
        res[k] = {"ms_median": round(med, 4), "ms_best": round(min(ts[k]), 4),
                  "ms_p90": round(float(np.percentile(ts[k], 90)), 4), "gbytes": round(nbytes[k] / 1e9, 3),
                  "tb_per_s": round(nbytes[k] / med / 1e9, 3)}
    for k in calls:
        res[k]["over_stack_sum"] = round(res[k]["ms_median"] / res["stack_sum"]["ms_median"], 4)
        res[k]["over_gradient_sums"] = round(res[k]["ms_median"] / res["gradient_sums"]["ms_median"], 4)
    # the planes of a last call against torch on a few columns
    _lib.check(calls["temporal_sums_8"]())
    torch.cuda.synchronize()
    y0, y1, x0, x1 = region
    cols = torch.arange(x0, x1 - 1, 257, device=dev)
    s16, rows_ = stack.view(torch.int16), slice(y0, y1 - 1)  # torch indexes int16, not uint16
    u = lambda t: t.to(torch.int64) & 0xFFFF  # noqa: E731
    a = u(s16[:, rows_][:, :, cols])
    ok = torch.equal(planes[0][rows_][:, cols], a.sum(0)) and torch.equal(planes[1][rows_][:, cols], (a * a).sum(0))
    for k, (dy, dx) in enumerate(summary.PARTNERS):
        if dx < 0:
            continue  # the first column's left partner may be outside: checked by the tests
        b = u(s16[:, y0 + dy:y1 - 1 + dy][:, :, cols + dx])
        ok = ok and torch.equal(planes[2 + k][rows_][:, cols], (a * b).sum(0))
    ok = ok and torch.equal(u(top.view(torch.int16)[rows_][:, cols]), a.max(0).values)
    res["temporal_sums_spot_check"] = bool(ok)
    return res


def finish(a, dev):
    H, W = (int(v) for v in a.size.split("x"))
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 65536, (16, H, W)).astype(np.uint16)
    frames = torch.from_numpy(frames.view(np.int16)).to(dev).view(torch.uint16)
    region = (6, H - 6, 7, W - 6)
    n, planes, top = summary.temporal_sums(frames, region, None, 8)
    planes = planes.cpu().numpy()
    out = {"size": [H, W], "region": list(region), "frames": n, "neighbours": 8}
    t0 = time.perf_counter()
    mean = summary.mean_image(planes, n, region)
    t1 = time.perf_counter()
    summary.std_image(planes, n, region)
    t2 = time.perf_counter()
    corr = summary.correlation_image(planes, n, region)
    t3 = time.perf_counter()
    summary.crispness(mean, region)
    t4 = time.perf_counter()
    out.update(mean_ms=round((t1 - t0) * 1e3, 1), std_ms=round((t2 - t1) * 1e3, 1),
               correlation_ms=round((t3 - t2) * 1e3, 1), crispness_ms=round((t4 - t3) * 1e3, 1),
               total_ms=round((t4 - t0) * 1e3, 1), mean_local_correlation=round(float(np.nanmean(corr)), 6))
    return out


def subpixel_scene(frames, noise, seed=31):
    """Crops of one blocky scene at shifts in steps of 1 / up px (box averages of a scene sampled
    ``up`` times finer) with independent Gaussian noise per frame; the middle frame unshifted."""
    rng = np.random.default_rng(seed)
    H, W, up = 200, 260, 4
    lo = rng.integers(0, 60000, (H // 4 + 16, W // 4 + 16)).astype(np.float64)
    fine = np.kron(lo, np.ones((4 * up, 4 * up)))  # `up` samples per pixel
    shifts = rng.integers(-6 * up, 6 * up + 1, (frames, 2))
    shifts[frames // 2] = 0
    imgs = []
    for dy, dx in shifts:
        oy, ox = 24 * up + int(dy), 24 * up + int(dx)
        crop = fine[oy:oy + H * up, ox:ox + W * up].reshape(H, up, W, up).mean(axis=(1, 3))
        imgs.append(crop)
    imgs = np.stack(imgs) + rng.normal(0, noise, (frames, H, W))
    return np.clip(imgs, 0, 65535).astype(np.uint16), shifts / up


def crispness(a):
    imgs, shifts = subpixel_scene(a.frames, a.noise)
    out = {"frames": a.frames, "size": list(imgs.shape[1:]), "noise_sigma": a.noise,
           "note": "one synthetic stack; the figures depend on the data"}
    for interp in ("linear", "cubic"):
        class VA(VideoAligner):
            DEVICES = [0]
            SUMMARY_IMAGES = True
            WARP_INTERPOLATION = interp

        va = VA()
        try:
            _, eu, skipped = va.align_images(imgs, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
        except (VideoAligner.AlignmentError, ValueError) as e:  # a result of the measurement too
            out[interp] = {"error": f"{type(e).__name__}: {e}"}
            continue
        err = eu[:, :2] - shifts[:, ::-1]
        out[interp] = {"crispness": round(va.crispness, 3), "region": list(va.summary_region),
                       "mean_local_correlation": round(float(np.nanmean(va.correlation_image)), 6),
                       "mean_std": round(float(np.nanmean(va.std_image)), 3), "skipped": len(skipped),
                       "rms_translation_error_px": round(float(np.sqrt((err ** 2).sum(1).mean())), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c2,c3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--finish", action="store_true")
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--crispness", action="store_true")
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--noise", type=float, default=3000.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    if a.finish:
        print(json.dumps(finish(a, dev)))
    elif a.crispness:
        print(json.dumps(crispness(a)))
    else:
        out = {"lib": os.environ.get("KCMC_LIB_PATH", "in-tree"), "reps": a.reps, "inner": a.inner}
        for name in a.shapes.split(","):
            out[name] = rates(name, a.reps, a.inner, dev)
            torch.cuda.empty_cache()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
