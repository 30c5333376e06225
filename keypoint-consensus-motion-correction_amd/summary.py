"""Summary images of an aligned uint16 stack (csrc/temporal_sums.hip): what motion-correction
pipelines hand on and judge a registration by, beside kcmc_amd.quality's mean image and
per-frame correlations.

  temporal_sums      kcmc_temporal_sums_u16: per pixel over time, exact 64-bit integer sums
                     of the pixel, its square and its products with 2 or 4 neighbours, and
                     the maximum -- one read of the stack
  mean_image         the rounded mean over time
  std_image          the temporal (population) standard deviation
  correlation_image  each pixel's mean Pearson correlation over time with its 4 or 8
                     neighbours (CaImAn's local_correlations, Suite2p's Vcorr)
  crispness          the norm of the mean image's gradient (NoRMCorre's figure)

The pass over the stack is a HIP kernel; the finishing functions are host arithmetic on its
planes (numpy arrays, no GPU needed), exact where it is integer: every numerator and
variance is an exact integer that is rounded to float64 once, as in quality.pearson.

Grayscale stacks [F, H, W] only; ``frames`` is one device tensor or the slabs of one stack
on several devices (as quality.stack_sum takes them).
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._intensity import Frames, Region, _slabs  # noqa: F401  (Frames, Region: this module's API)
from .quality import _selection
from .stages import _aligned16, _ctx, _device_of, _ptr, _stream

# (dy, dx) of the partner of planes 2, 3, 4, 5 (include/kcmc.h)
PARTNERS = ((0, 1), (1, 0), (1, 1), (1, -1))


def check_neighbours(neighbours) -> int:
    if isinstance(neighbours, bool) or neighbours not in (4, 8):
        raise ValueError(f"neighbours must be 4 or 8, got {neighbours!r}")
    return int(neighbours)


def _u16_max(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """maximum of two uint16 tensors through their int16 views (x ^ 0x8000 maps the order of
    uint16 onto int16's)."""
    m = torch.maximum(a.view(torch.int16) ^ -32768, b.view(torch.int16) ^ -32768)
    return (m ^ -32768).view(torch.uint16)


def temporal_sums(frames: Frames, region: Region, sel=None, neighbours: int = 8
                  ) -> Tuple[int, torch.Tensor, torch.Tensor]:
    """(n, planes [K, H, W] int64, max [H, W] uint16) over the frames with ``sel`` set (a host
    bool array over all frames; None = every frame) and the pixels of ``region`` = (y0, y1,
    x0, x1); n the number of selected frames, K = 2 + neighbours / 2, the planes as
    include/kcmc.h lays them out (sum a, sum a^2, sum a * right, sum a * down, and with 8
    neighbours sum a * down-right, sum a * down-left); 0 outside the region.  Per-slab planes
    are added and per-slab maxima combined on the first slab's device."""
    parts = _slabs(frames)
    H, W = parts[0].shape[1:]
    if H * W == 0:
        raise ValueError("empty frames")
    neighbours = check_neighbours(neighbours)
    K = 2 + neighbours // 2
    y0, y1, x0, x1 = (int(v) for v in region)
    n_frames = sum(p.shape[0] for p in parts)
    sel = _selection(sel, n_frames)
    L = _lib.load()
    outs, f0 = [], 0
    for p in parts:  # queued on every device before the planes are brought together
        dev = _device_of(p)
        with torch.cuda.device(dev):
            planes = torch.empty((K, H, W), dtype=torch.int64, device=dev)
            # the kernel updates the max image in 32-bit words: an even number of elements
            mx = torch.empty(H * W + (H * W & 1), dtype=torch.uint16, device=dev)
            s = None
            if sel is not None:
                s = torch.from_numpy(np.ascontiguousarray(sel[f0:f0 + p.shape[0]]).view(np.uint8)).to(dev)
            _lib.check(L.kcmc_temporal_sums_u16(_ctx(dev).handle, _ptr(_aligned16(p)), p.shape[0], H, W, _ptr(s),
                                                y0, y1, x0, x1, neighbours, _ptr(planes), _ptr(mx), _stream(dev)))
        outs.append((planes, mx[:H * W].view(H, W)))
        f0 += p.shape[0]
    total, top = outs[0]
    for planes, mx in outs[1:]:
        total = total + planes.to(total.device)
        top = _u16_max(top, mx.to(top.device))
    return (n_frames if sel is None else int(sel.sum())), total, top


# ------------------------------------------------------------------ the finishing functions
def _planes(planes, n, region):
    """(the planes cut to the region, in the integer type their arithmetic is exact in; n;
    (H, W); the region).  By Cauchy-Schwarz every term of the formulas below -- n * S1, S0^2,
    n * Spq, Sp * Sq -- is bounded by n * max(S1): below 2^63 the arithmetic runs vectorised in
    int64, from there on on Python ints (object arrays)."""
    planes = np.asarray(planes)
    if planes.ndim != 3 or planes.shape[0] not in (4, 6) or planes.dtype.kind not in "iuO":
        raise ValueError(f"planes must be [4 or 6, H, W] integers, got {planes.dtype} {planes.shape}")
    n = int(n)
    if n <= 0:
        raise ValueError("no frame selected")
    H, W = planes.shape[1:]
    y0, y1, x0, x1 = (int(v) for v in region)
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"region {region} is empty or outside the {H} x {W} image")
    big = n * int(planes[1].max()) >= 1 << 63
    cut = planes[:, y0:y1, x0:x1].astype(object if big else np.int64)
    return cut, n, (H, W), (y0, y1, x0, x1)


def _placed(values, shape, region, fill, dtype):
    out = np.full(shape, fill, dtype)
    y0, y1, x0, x1 = region
    out[y0:y1, x0:x1] = values
    return out


def mean_image(planes, n: int, region: Region) -> np.ndarray:
    """(S0 + n // 2) // n inside the region, 0 outside: [H, W] uint16."""
    P, n, shape, region = _planes(planes, n, region)
    return _placed(((P[0] + n // 2) // n).astype(np.uint16), shape, region, 0, np.uint16)


def _variance(P, n):
    return n * P[1] - P[0] * P[0]  # exact, >= 0


def std_image(planes, n: int, region: Region) -> np.ndarray:
    """The population standard deviation over time, sqrt(float(n * S1 - S0^2)) / n with the
    radicand an exact integer: [H, W] float64, NaN outside the region.  (On Python ints when
    n * max(S1) >= 2^63: slow.)"""
    P, n, shape, region = _planes(planes, n, region)
    return _placed(np.sqrt(_variance(P, n).astype(np.float64)) / n, shape, region, np.nan, np.float64)


def correlation_image(planes, n: int, region: Region) -> np.ndarray:
    """Each pixel's mean Pearson correlation over time with its neighbours (4 for four
    planes, 8 for six): [H, W] float64, NaN outside the region.

    For a pixel p and each existing neighbour q, both inside the region,
        r = float(n Spq - Sp Sq) / (sqrt(float(n Spp - Sp^2)) * sqrt(float(n Sqq - Sq^2)))
    -- quality.pearson's arithmetic: integers exact, one rounding per term, no clamping (two
    identical series may give 1.0000000000000002).  A pair with a zero variance on either
    side is left out.  The pixel's value is the float64 sum of its remaining r's in the
    order right, left, down, up, down-right, up-left, down-left, up-right, divided by their
    count; NaN when no pair remains.  (On Python ints when n * max(S1) >= 2^63: slow.)"""
    P, n, shape, region = _planes(planes, n, region)
    h, w = P.shape[1:]
    var = _variance(P, n)
    live = var != 0
    sd = np.sqrt(var.astype(np.float64))
    total, count = np.zeros((h, w)), np.zeros((h, w), np.int64)
    for k, (dy, dx) in enumerate(PARTNERS[:P.shape[0] - 2]):
        # p over the pixels whose partner q = p + (dy, dx) is inside the region
        p = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
        q = (slice(dy, h), slice(max(0, dx), w + min(0, dx)))
        num = (n * P[2 + k][p] - P[0][p] * P[0][q]).astype(np.float64)
        both = live[p] & live[q]
        r = np.divide(num, sd[p] * sd[q], out=np.zeros_like(num), where=both)
        for at in (p, q):  # the pair counts for p (right, down, ...) and then for q (left, up, ...)
            total[at] += r
            count[at] += both
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(count > 0, total / count, np.nan)
    return _placed(out, shape, region, np.nan, np.float64)


def crispness(mean_u16, region: Region) -> float:
    """sqrt(sum(gx^2 + gy^2)) / 2 over the region shrunk by one pixel on every side, with
    gx = m[y, x + 1] - m[y, x - 1] and gy = m[y + 1, x] - m[y - 1, x] as integers: the
    Frobenius norm of np.gradient's magnitude of the mean image there.  NaN when the shrunk
    region is empty."""
    m = np.asarray(mean_u16)
    if m.ndim != 2 or m.dtype != np.uint16:
        raise ValueError("mean_u16 must be [H, W] uint16")
    y0, y1, x0, x1 = (int(v) for v in region)
    if not (0 <= y0 <= y1 <= m.shape[0] and 0 <= x0 <= x1 <= m.shape[1]):
        raise ValueError(f"region {region} is outside the {m.shape[0]} x {m.shape[1]} image")
    if y1 - y0 < 3 or x1 - x0 < 3:
        return math.nan
    m = m.astype(np.int64)
    gx = m[y0 + 1:y1 - 1, x0 + 2:x1] - m[y0 + 1:y1 - 1, x0:x1 - 2]
    gy = m[y0 + 2:y1, x0 + 1:x1 - 1] - m[y0:y1 - 2, x0 + 1:x1 - 1]
    rows = (gx * gx + gy * gy).sum(axis=1)  # each < 2^34 * W; their total may pass 2^63
    return math.sqrt(float(sum(int(v) for v in rows))) / 2
