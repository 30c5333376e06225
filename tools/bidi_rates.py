"""The two kernels of the bidirectional-scan phase correction (csrc/bidi_phase.hip) timed with HIP
events on one device.

    python tools/bidi_rates.py [--frames 2000] [--reps 10] [--shift 3] [--radius 8] [--sample 64]

Row shift: kcmc_shift_rows_u16 on a stack of `frames` frames of 1080 x 1920, out of place (every
row is read and written: the bytes of a copy) and in place (only the odd rows move: half the
bytes each way), beside Tensor.copy_ of the same stack in the same run -- the yardstick for bytes
moved.  Phase sums: kcmc_bidi_phase_sums_u16 at `radius` on `sample` frames of the stack
(bidi.sample_indices, gathered into one tensor) beside kcmc_frame_stats_u16 on the same frames
against their first frame over the whole image, which reads the same bytes once and forms one
product per pixel where the phase sums form 2 radius + 1.

The C entry points are called directly into preallocated outputs; a timed window is one call
between two events, the calls in alternation after a warm-up of each, `reps` times.  Three frames
of the shifted stack and the sums of three frames are compared with torch.  Prints one JSON
line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kcmc_amd import _lib, bidi, stages  # noqa: E402
from refine_rates import H, W, timed  # noqa: E402


def shifted_by_torch(fr, d):
    fr = fr.view(torch.int16)  # torch indexes and compares int16, not uint16: the bits are the same
    out = fr.clone()
    cols = (torch.arange(W, device=fr.device) + d).clamp_(0, W - 1)
    out[:, 1::2] = fr[:, 1::2][:, :, cols]
    return out


def sums_by_torch(fr, R):
    """bidi's sums of one frame [H, W] in int64 on the device."""
    x = fr.view(torch.int16).to(torch.int64) & 0xFFFF
    odd = torch.tensor([y if y & 1 else y + 1 for y in range(H - 1)], device=fr.device)
    even = torch.tensor([y + 1 if y & 1 else y for y in range(H - 1)], device=fr.device)
    b = x[even, R:W - R]
    rows = []
    for d in range(-R, R + 1):
        a = x[odd, R + d:W - R + d]
        rows.append(torch.stack([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()]))
    return torch.stack(rows)


def summary(v, nbytes):
    med = float(np.median(v))
    return {"ms_median": round(med, 3), "ms_best": round(min(v), 3), "ms_p90": round(float(np.percentile(v, 90)), 3),
            "gb_per_s": round(nbytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shift", type=int, default=3)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--sample", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    F, d, R = a.frames, a.shift, a.radius
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    for f0 in range(0, F, 100):  # full-range noise: the content does not change what is moved
        n = min(F, f0 + 100) - f0
        src[f0:f0 + n] = torch.randint(-32768, 32768, (n, H, W), dtype=torch.int16, device=dev).view(torch.uint16)
    dst = torch.empty_like(src)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr

    def copy():
        dst.copy_(src)
        return _lib.KCMC_OK

    # in place the stack is shifted back and forth: every call moves the same bytes
    sign = [d]

    def in_place():
        sign[0] = -sign[0]
        return L.kcmc_shift_rows_u16(ctx, ptr(dst), ptr(dst), F, H, W, 1, sign[0], st)

    calls = {"copy_": copy,
             "shift_out_of_place": lambda: L.kcmc_shift_rows_u16(ctx, ptr(src), ptr(dst), F, H, W, 1, d, st),
             "shift_in_place": in_place}
    ts = {k: [] for k in calls}
    for k in calls:
        for _ in range(2):
            _lib.check(calls[k]())
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
            ts[k].append(timed(calls[k]))
    stack_bytes = 2 * F * H * W
    res = {"shape": [F, H, W], "shift": d, "reps": a.reps,
           "copy_": summary(ts["copy_"], 2 * stack_bytes),
           "shift_out_of_place": summary(ts["shift_out_of_place"], 2 * stack_bytes),
           "shift_in_place": summary(ts["shift_in_place"], stack_bytes)}  # H even: half the rows, read and written
    res["out_of_place_over_copy"] = round(res["shift_out_of_place"]["ms_median"] / res["copy_"]["ms_median"], 3)
    res["in_place_over_copy"] = round(res["shift_in_place"]["ms_median"] / res["copy_"]["ms_median"], 3)
    _lib.check(calls["shift_out_of_place"]())
    spot = [0, F // 2, F - 1]
    picked = torch.stack([src[f] for f in spot])
    want = shifted_by_torch(picked, d)
    res["shift_equals_torch"] = bool(torch.equal(torch.stack([dst[f] for f in spot]).view(torch.int16), want))
    _lib.check(L.kcmc_shift_rows_u16(ctx, ptr(picked), ptr(picked), len(spot), H, W, 1, d, st))
    res["in_place_equals_torch"] = bool(torch.equal(picked.view(torch.int16), want))
    del dst

    idx = bidi.sample_indices(F, a.sample)
    K = len(idx)
    sample = torch.stack([src[f] for f in idx])
    ref = sample[0].contiguous()
    sums = torch.empty((K, 2 * R + 1, 5), dtype=torch.int64, device=dev)
    stats = torch.empty((K, 5), dtype=torch.int64, device=dev)
    calls = {"phase_sums": lambda: L.kcmc_bidi_phase_sums_u16(ctx, ptr(sample), K, H, W, None, K, R, ptr(sums), st),
             "frame_stats": lambda: L.kcmc_frame_stats_u16(ctx, ptr(sample), K, H, W, ptr(ref), 0, H, 0, W, ptr(stats),
                                                           st)}
    ts = {k: [] for k in calls}
    for k in calls:
        for _ in range(2):
            _lib.check(calls[k]())
    torch.cuda.synchronize()
    for rep in range(a.reps):
        for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
            ts[k].append(timed(calls[k]))
    res["sample"] = K
    res["radius"] = R
    res["phase_sums"] = summary(ts["phase_sums"], 2 * K * H * W)
    res["frame_stats"] = summary(ts["frame_stats"], 2 * K * H * W)
    res["phase_sums_over_frame_stats"] = round(res["phase_sums"]["ms_median"] / res["frame_stats"]["ms_median"], 3)
    res["sums_equal_torch"] = all(bool(torch.equal(sums[k], sums_by_torch(sample[k], R))) for k in (0, K // 2, K - 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
