"""The box band-pass prefilter (csrc/band_filter.hip) timed with HIP events on one device.

    python tools/prefilter_rates.py [--reps 10] [--shapes 2000x1080x1920,2500x512x512]

kcmc_box_bandpass_u16 at the radii (1, 12) and (4, 32) on a stack of config 2's shape (2000 x 1080 x
1920) and of config 3's (2500 x 512 x 512), beside the two yardsticks that read and write the same
bytes once: Tensor.copy_ of the stack and the out-of-place kcmc_shift_rows_u16.  The copy is the
floor.

The C entry points are called directly into one preallocated output; a timed window is one call
between two events, the calls in alternation after a warm-up of each, `reps` times; the median
is reported.  The first, a middle and the last frame of each filtered stack are compared with
the definition restated in torch (int64 integral images) -- at config 2's shape the last frame
lies beyond 2^31 elements and 2^32 bytes.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kcmc_amd import _lib, stages  # noqa: E402
from refine_rates import timed  # noqa: E402

RADII = ((1, 12), (4, 32))


def rounded_box_mean(a, rho):
    """m_rho of one int64 frame [H, W] on its device, from the integral image."""
    if rho == 0:
        return a
    H, W = a.shape
    I = torch.zeros((H + 1, W + 1), dtype=torch.int64, device=a.device)
    I[1:, 1:] = a.cumsum(0).cumsum(1)
    ys, xs = torch.arange(H, device=a.device), torch.arange(W, device=a.device)
    y0, y1 = (ys - rho).clamp_(min=0), (ys + rho).clamp_(max=H - 1) + 1
    x0, x1 = (xs - rho).clamp_(min=0), (xs + rho).clamp_(max=W - 1) + 1
    S = I[y1][:, x1] - I[y0][:, x1] - I[y1][:, x0] + I[y0][:, x0]
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return (S + n // 2) // n


def bandpass_by_torch(frame, s, r):
    """The definition of include/kcmc.h for one uint16 frame; int64 [H, W]."""
    a = frame.view(torch.int16).to(torch.int64) & 0xFFFF
    m = rounded_box_mean(a, s)
    if r > 0:
        m = m - rounded_box_mean(a, r)
    return m.clamp_(min=0)


def summary(v, nbytes):
    med = float(np.median(v))
    return {"ms_median": round(med, 3), "ms_best": round(min(v), 3), "ms_p90": round(float(np.percentile(v, 90)), 3),
            "gb_per_s": round(nbytes / med / 1e6, 1)}


def rates(F, H, W, reps, dev):
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    step = max(1, (100 * 1080 * 1920) // (H * W))
    for f0 in range(0, F, step):  # full-range noise: the content does not change what is moved
        n = min(F, f0 + step) - f0
        src[f0:f0 + n] = torch.randint(-32768, 32768, (n, H, W), dtype=torch.int16, device=dev).view(torch.uint16)
    dst = torch.empty_like(src)
    L = _lib.load()
    ctx, st, ptr = stages._ctx(dev).handle, stages._stream(dev), stages._ptr

    def copy():
        dst.copy_(src)
        return _lib.KCMC_OK

    def bandpass(s, r):
        return lambda: L.kcmc_box_bandpass_u16(ctx, ptr(src), ptr(dst), F, H, W, s, r, st)

    calls = {"copy_": copy,
             "shift_out_of_place": lambda: L.kcmc_shift_rows_u16(ctx, ptr(src), ptr(dst), F, H, W, 1, 3, st)}
    calls.update({f"bandpass_{s}_{r}": bandpass(s, r) for s, r in RADII})
    ts = {k: [] for k in calls}
    for k in calls:
        for _ in range(2):
            _lib.check(calls[k]())
    torch.cuda.synchronize()
    for rep in range(reps):
        for k in (list(calls) if rep % 2 == 0 else list(calls)[::-1]):
            ts[k].append(timed(calls[k]))
    nbytes = 2 * 2 * F * H * W  # the stack read once and written once
    res = {"shape": [F, H, W], "elements": F * H * W, "reps": reps}
    res.update({k: summary(v, nbytes) for k, v in ts.items()})
    for s, r in RADII:
        k = f"bandpass_{s}_{r}"
        res[k + "_over_copy"] = round(res[k]["ms_median"] / res["copy_"]["ms_median"], 3)
        res[k + "_over_shift"] = round(res[k]["ms_median"] / res["shift_out_of_place"]["ms_median"], 3)
        _lib.check(calls[k]())
        res[k + "_equals_torch"] = all(
            bool(torch.equal(dst[f].view(torch.int16).to(torch.int64) & 0xFFFF, bandpass_by_torch(src[f], s, r)))
            for f in (0, F // 2, F - 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="2000x1080x1920,2500x512x512")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: nothing is measured without one")
    dev = torch.device("cuda", 0)
    for shape in a.shapes.split(","):
        F, H, W = (int(v) for v in shape.split("x"))
        print(json.dumps(rates(F, H, W, a.reps, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
