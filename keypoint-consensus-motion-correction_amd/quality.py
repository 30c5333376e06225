"""Registration quality metrics of an aligned uint16 stack (csrc/quality.hip).

What every motion-correction tool reports after registration: the mean image of the
aligned frames, the region that is valid in every frame, and each frame's Pearson
correlation with the mean image over that region.  The two passes over the stack are HIP
kernels (exact 64-bit integer sums); what is left -- the rounded mean, the region, the
correlation from the five integer moments, the choice of the best-registered frames for a
refined template -- is small host arithmetic, exact where it is integer.

  stack_sum / mean_image            kcmc_stack_sum_u16
  frame_stats / frame_correlations  kcmc_frame_stats_u16 + pearson
  valid_region                      from the forward maps, as the warp inverts them
  select_top                        the frames a refined template is averaged from

Grayscale stacks [F, H, W] only; ``frames`` is one device tensor or the slabs of one stack
on several devices (as stages.brightest_px takes them).  Homographies are out of scope:
their displacement field is not bounded by its values at the image corners.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._intensity import Frames, Region, _slabs, ref_tensor  # noqa: F401  (Frames, Region: this module's API)
from .stages import _aligned16, _ctx, _device_of, _ptr, _stream


def _selection(sel, n_frames: int) -> Optional[np.ndarray]:
    if sel is None:
        return None
    sel = np.asarray(sel)
    if sel.dtype != np.bool_ or sel.shape != (n_frames,):
        raise ValueError(f"sel must be a bool array over all {n_frames} frames")
    return sel


def stack_sum(frames: Frames, sel=None) -> torch.Tensor:
    """The exact per-pixel sum [H, W] int64 over the frames with ``sel`` set (a host bool
    array over all frames; None = every frame).  Per-slab sums are added on the first
    slab's device."""
    parts = _slabs(frames)
    H, W = parts[0].shape[1:]
    if H * W == 0:
        raise ValueError("empty frames")
    sel = _selection(sel, sum(p.shape[0] for p in parts))
    L = _lib.load()
    sums, f0 = [], 0
    for p in parts:  # queued on every device before the sums are brought together
        dev = _device_of(p)
        with torch.cuda.device(dev):
            out = torch.empty((H, W), dtype=torch.int64, device=dev)
            s = None
            if sel is not None:
                s = torch.from_numpy(np.ascontiguousarray(sel[f0:f0 + p.shape[0]]).view(np.uint8)).to(dev)
            _lib.check(L.kcmc_stack_sum_u16(_ctx(dev).handle, _ptr(_aligned16(p)), p.shape[0], H * W, _ptr(s), _ptr(out),
                                            _stream(dev)))
        sums.append(out)
        f0 += p.shape[0]
    total = sums[0]
    for s in sums[1:]:
        total = total + s.to(total.device)
    return total


def mean_image(frames: Frames, sel=None) -> torch.Tensor:
    """(sum + n // 2) // n of the selected frames, [H, W] uint16 on the first slab's device;
    ValueError when no frame is selected."""
    parts = _slabs(frames)
    n_frames = sum(p.shape[0] for p in parts)
    n = n_frames if sel is None else int(_selection(sel, n_frames).sum())
    if n == 0:
        raise ValueError("mean_image: no frame selected")
    total = stack_sum(parts, sel)
    mean = (total.cpu().numpy() + n // 2) // n  # <= 65535: the rounded mean of uint16 values
    return torch.from_numpy(mean.astype(np.uint16)).to(total.device)


def _invert_affines(affines: np.ndarray) -> np.ndarray:
    """The warp's (OpenCV warpAffine's) inversion of forward maps [F, 2, 3], in float64 and
    in its order of operations (csrc/warp.hip invert_affine)."""
    M = np.array(affines, dtype=np.float64, copy=True)
    D = M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    with np.errstate(divide="ignore"):
        D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
    A11, A22 = M[:, 1, 1] * D, M[:, 0, 0] * D
    M[:, 0, 0] = A11
    M[:, 0, 1] *= -D
    M[:, 1, 0] *= -D
    M[:, 1, 1] = A22
    b1 = -M[:, 0, 0] * M[:, 0, 2] - M[:, 0, 1] * M[:, 1, 2]
    b2 = -M[:, 1, 0] * M[:, 0, 2] - M[:, 1, 1] * M[:, 1, 2]
    M[:, 0, 2] = b1
    M[:, 1, 2] = b2
    return M


def valid_region(affines: np.ndarray, H: int, W: int, taps: int = 2) -> Region:
    """(y0, y1, x0, x1): the rectangle [m, H - m) x [m, W - m) whose pixels no frame's warp
    fills from outside the source image.  m = ceil(d) + 1, d the largest displacement
    |M_f^-1(c) - c| (max norm) over the frames and the four corners c of the pixel rectangle:
    the displacement field of an affine map is affine, so its maximum over the image is at
    a corner; the + 1 covers the second bilinear tap and the warp's 1/32 px fixed point.

    d is evaluated in float64, and the last bit of an estimated map must not cost a pixel of
    margin (a rotation of 3.5e-18 rad beside an exact shift of 6 px evaluates to
    6.000000000000001 at one corner), so a displacement up to (H + W) * 2^-40 px above an
    integer counts as that integer.  That is far above float64's rounding of these few
    products and sums and far below what the margin needs: x in [m, W - 1 - m] reads source
    column x + disp, rounded to the fixed point by less than 1/16 px, and both taps are inside
    while that lies in [0, W - 1), i.e. while m > d + 1/16; m >= d - tol + 1 keeps that.

    taps = 4 (the bicubic warp, K3c): m = ceil(d - tol) + 2.  The footprint reaches one pixel
    further on each side: a pixel whose fixed-point source column is c reads columns
    floor(c) - 1 .. floor(c) + 2, all inside the image (an interior pixel of the definition)
    while c lies in [1, W - 2).  For x in [m, W - 1 - m], c is within d + 1/16 of x, so that
    holds while m > d + 1 + 1/16, and m >= d - tol + 2 keeps it; the same in y."""
    if taps not in (2, 4):
        raise ValueError(f"valid_region: taps must be 2 (bilinear) or 4 (bicubic), got {taps!r}")
    a = np.asarray(affines, dtype=np.float64)
    if a.ndim == 3 and a.shape[1:] == (3, 3):
        raise NotImplementedError("valid_region: homographies are not supported (a projective displacement field "
                                  "is not bounded by its corners)")
    if a.ndim != 3 or a.shape[1:] != (2, 3):
        raise ValueError(f"affines must be [F, 2, 3], got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError("valid_region: non-finite affine")
    H, W = int(H), int(W)
    d = 0.0
    if len(a):
        inv = _invert_affines(a)
        corners = np.array([[0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0]])
        mapped = np.einsum("fij,cj->fci", inv[:, :, :2], corners) + inv[:, None, :, 2]
        d = float(np.abs(mapped - corners[None]).max())
        if not math.isfinite(d):
            raise ValueError("valid_region: non-finite displacement")
    m = math.ceil(d - (H + W) * 2.0 ** -40) + taps // 2
    if 2 * m >= min(H, W):
        raise ValueError("no common valid region")
    return m, H - m, m, W - m


def frame_stats(frames: Frames, ref, region: Region) -> np.ndarray:
    """[F, 5] int64 = (sum a, sum b, sum a^2, sum b^2, sum a*b) over ``region`` = (y0, y1, x0, x1)
    for every frame a against the reference image b ([H, W] uint16, copied to every slab's
    device)."""
    parts = _slabs(frames)
    H, W = parts[0].shape[1:]
    y0, y1, x0, x1 = (int(v) for v in region)
    ref_t = ref_tensor(ref, H, W)
    L = _lib.load()
    outs = []
    for p in parts:
        dev = _device_of(p)
        with torch.cuda.device(dev):
            out = torch.empty((p.shape[0], 5), dtype=torch.int64, device=dev)
            r = _aligned16(ref_t.to(dev).contiguous())
            _lib.check(L.kcmc_frame_stats_u16(_ctx(dev).handle, _ptr(_aligned16(p)), p.shape[0], H, W, _ptr(r), y0, y1,
                                              x0, x1, _ptr(out), _stream(dev)))
        outs.append(out)
    return np.concatenate([o.cpu().numpy() for o in outs])


def pearson(stats: np.ndarray, n: int) -> np.ndarray:
    """Pearson's r [F] float64 from frame_stats' moments over ``n`` pixels.  Numerator and
    variances in exact integers (Python ints: n * sum(ab) exceeds 2^63), one rounding each to
    float64, then r = num / (sqrt(va) * sqrt(vb)); NaN for a constant frame or reference."""
    stats = np.asarray(stats)
    n = int(n)
    out = np.full(len(stats), np.nan)
    for f, row in enumerate(stats):
        sa, sb, saa, sbb, sab = (int(v) for v in row)
        va = n * saa - sa * sa
        vb = n * sbb - sb * sb
        if va != 0 and vb != 0:
            out[f] = float(n * sab - sa * sb) / (math.sqrt(float(va)) * math.sqrt(float(vb)))
    return out


def frame_correlations(frames: Frames, ref, region: Region) -> np.ndarray:
    """Every frame's Pearson correlation with ``ref`` over ``region``: [F] float64."""
    y0, y1, x0, x1 = region
    return pearson(frame_stats(frames, ref, region), (y1 - y0) * (x1 - x0))


def select_top(corr: np.ndarray, candidates: Sequence[int], top_frac: float) -> List[int]:
    """The best-registered candidates: ordered by (-corr, index) with NaN as -inf, the first
    max(1, ceil(top_frac * len(candidates))) of them."""
    cand = [int(i) for i in candidates]
    if not cand:
        raise ValueError("select_top: no candidate frame")
    key = lambda i: (-(corr[i] if not math.isnan(corr[i]) else -math.inf), i)  # noqa: E731
    return sorted(cand, key=key)[:max(1, math.ceil(top_frac * len(cand)))]
