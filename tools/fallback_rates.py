"""The shift-search kernel (csrc/shift_search.hip) timed with HIP events beside the plain torch
formulation of the same sums, and the cost of the whole opt-in fallback pass.

    python tools/fallback_rates.py [--reps 10]
    python tools/fallback_rates.py --pass [--frames 2000] [--rounds 7]

Rates: 16 frames at 512 x 512 and at 1080 x 1920 against one reference image, R = 8 and R = 16,
the rectangle a pass with shifts up to 5 px would use (the valid region shrunk by R).  The C
entry point is called directly into a preallocated output; a timed window is one call between
two events after a warm-up of the same shape, `reps` times.  The torch formulation is what a
user would write without the kernel -- per shift a sliced view of the frames, an int64
multiply and a sum -- on the same device and data, timed once per shape after a warm-up of a
few shifts (it takes (2R + 1)^2 passes); its result must equal the kernel's.

--pass: align_keypoints on a config-2-shaped device-resident stack (1080 x 1920, 500 template
keypoints) with 1 % of the frames blind (every descriptor one row: no model), FALLBACK off and
on in alternation; the difference is the whole pass (mean image, search, re-warp, host
arithmetic).

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
from kcmc_amd import VideoAligner, _lib, stages, synthetic  # noqa: E402


def _i64(t):
    """uint16 -> int64 on the device through the int16 view (torch converts int16 everywhere)."""
    return t.view(torch.int16).to(torch.int64) & 0xFFFF


def torch_search(frames, ref, rect, R):
    """[F, S, S, 5] int64 the plain way: per shift a sliced view, an int64 multiply, a sum."""
    y0, y1, x0, x1 = rect
    F, S = frames.shape[0], 2 * R + 1
    out = torch.empty((F, S, S, 5), dtype=torch.int64, device=frames.device)
    b = _i64(ref[y0:y1, x0:x1])
    out[..., 1] = b.sum()
    out[..., 3] = (b * b).sum()
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            a = _i64(frames[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx])
            out[:, dy + R, dx + R, 0] = a.sum((1, 2))
            out[:, dy + R, dx + R, 2] = (a * a).sum((1, 2))
            out[:, dy + R, dx + R, 4] = (a * b).sum((1, 2))
    return out


def rates(H, W, R, reps, dev, F=16):
    base = synthetic.make_texture((H, W), seed=7)
    rng = np.random.default_rng(3)
    fr = np.stack([np.roll(base, (int(a), int(b)), axis=(0, 1)) for a, b in rng.integers(-5, 6, (F, 2))])
    frames = torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
    ref = torch.from_numpy(np.ascontiguousarray(base)).to(dev).contiguous()  # row-major, as the entry point reads it
    m = 6 + R  # valid region of shifts <= 5 px, shrunk by R
    rect = (m, H - m, m, W - m)
    S = 2 * R + 1
    out = torch.empty((F, S, S, 5), dtype=torch.int64, device=dev)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr
    args = (ctx, ptr(frames), F, H, W, None, F, ptr(ref), *rect, R, ptr(out), st)
    call = lambda: L.kcmc_shift_search_u16(*args)  # noqa: E731
    for _ in range(2):
        _lib.check(call())
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(call())
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    torch_search(frames[:2], ref, rect, 1)  # warm-up of the torch kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = torch_search(frames, ref, rect, R)
    torch.cuda.synchronize()
    t_torch = (time.perf_counter() - t0) * 1e3
    n = (rect[1] - rect[0]) * (rect[3] - rect[2])
    med = float(np.median(ts))
    return {"shape": [F, H, W], "R": R, "rect": list(rect), "kernel_ms_median": round(med, 4),
            "kernel_ms_best": round(min(ts), 4), "kernel_ms_p90": round(float(np.percentile(ts, 90)), 4),
            "torch_ms": round(t_torch, 2), "torch_over_kernel": round(t_torch / med, 1),
            "gmacs": round(F * n * S * S / 1e9, 3), "tmacs_per_s": round(F * n * S * S / med / 1e9, 3),
            "equal": bool(torch.equal(out, want)),
            "mismatches_per_sum": [int((out[..., k] != want[..., k]).sum()) for k in range(5)]}


def whole_pass(a, dev):
    F, H, W, n_tpl = a.frames, 1080, 1920, 500
    ks = synthetic.make_keypoints(F, n_tpl, 32, (H, W), seed=3)
    rng = np.random.default_rng(11)
    blind = sorted(int(i) for i in rng.choice(np.arange(1, F - 1), max(1, F // 100), replace=False))
    for f in blind:
        lo, hi = ks.q_off[f], ks.q_off[f + 1]
        ks.des_q[lo:hi] = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    base = torch.from_numpy(synthetic.make_texture((H, W), seed=0)).to(dev)
    frames = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    gt = torch.from_numpy(ks.gt).to(dev)
    for f0 in range(0, F, 250):  # each frame: the texture seen through the inverse of its frame -> template map
        f1 = min(F, f0 + 250)
        src = base.expand((f1 - f0, H, W)).contiguous()
        stages.warp_affine_u16(src, gt[f0:f1].contiguous(), out=frames[f0:f1], inverse_map=True)
    kq = [ks.kp_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(F)]
    dq = [ks.des_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(F)]

    def aligner(mode):
        # QUALITY_METRICS publishes the maps (va.affines) in both modes; its cost is in both timings
        return type("VA", (VideoAligner,), {"DEVICES": [0], "FALLBACK": mode, "FALLBACK_RADIUS": a.radius,
                                            "QUALITY_METRICS": True})()

    ts = {"interpolate": [], "correlation": []}
    info = {}
    for rnd in range(a.rounds + 1):  # round 0 warms up
        for mode in (list(ts) if rnd % 2 == 0 else list(ts)[::-1]):
            va = aligner(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, skipped = va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=100)
            torch.cuda.synchronize()
            if rnd:
                ts[mode].append((time.perf_counter() - t0) * 1e3)
            c = np.array([(W - 1) / 2, (H - 1) / 2, 1.0])  # a shift corrects the map where the pixels are
            err = np.abs((va.affines[blind] - ks.gt[blind]) @ c)
            info[mode] = {"skipped": len(skipped), "blind_centre_error_px_median": round(float(np.median(err)), 3),
                          "blind_centre_error_px_max": round(float(err.max()), 3)}
            if mode == "correlation":
                ok = [blind.index(i) for i in va.fallback_idxs]
                info[mode].update(corrected=len(ok), corrected_centre_error_px_max=round(float(err[ok].max()), 3))
    off, on = float(np.median(ts["interpolate"])), float(np.median(ts["correlation"]))
    return {"shape": [F, H, W], "blind": len(blind), "radius": a.radius, "rounds": a.rounds,
            "off_ms": [round(t, 1) for t in ts["interpolate"]], "on_ms": [round(t, 1) for t in ts["correlation"]],
            "off_ms_median": round(off, 1), "on_ms_median": round(on, 1), "pass_ms": round(on - off, 1), **info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pass", dest="whole", action="store_true")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    if a.whole:
        print(json.dumps(whole_pass(a, dev)))
    else:
        print(json.dumps({"reps": a.reps, "runs": [rates(H, W, R, a.reps, dev)
                                                   for H, W in ((512, 512), (1080, 1920)) for R in (8, 16)]}))


if __name__ == "__main__":
    main()
