"""Bidirectional-scan phase correction (csrc/bidi_phase.hip).

A two-photon microscope that scans bidirectionally acquires the odd image rows on the return
sweep; an error in its line clock displaces every odd row horizontally against the even rows by
a constant.  The offset is not a motion -- no map the aligner fits can express it -- so it is
measured and undone before registration (VideoAligner.BIDI_PHASE).  Build-defined: the
reference has no such mode; the semantics are written down in include/kcmc.h and DESIGN.md
(b1) and restated in numpy in tests/test_bidi_host.py.

  phase_sums       kcmc_bidi_phase_sums_u16: the exact correlation moments of the odd rows read
                   at x + d against their even neighbours at x, for every d in [-R, R]
  sample_indices   the frames that are measured
  estimate_offset  the sums pooled over the frames, Pearson's r per d, the peak and its
                   rejection rules
  shift_rows       kcmc_shift_rows_u16: the rows of one parity moved by d columns, the edge
                   pixel replicated

Whole pixels only: up to half a pixel of the offset remains.  Grayscale stacks [F, H, W].
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import quality as _q
from ._intensity import Frames, _slabs
from .stages import _ctx, _device_of, _ptr, _require, _stream

MAX_RADIUS = 16
MAX_SHIFT = 16


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_radius(radius) -> int:
    if not (_is_int(radius) and 0 <= int(radius) <= MAX_RADIUS):
        raise ValueError(f"the phase radius must be an integer in [0, {MAX_RADIUS}], got {radius!r}")
    return int(radius)


def check_shift(d) -> int:
    if not (_is_int(d) and -MAX_SHIFT <= int(d) <= MAX_SHIFT):
        raise ValueError(f"the row shift must be an integer in [-{MAX_SHIFT}, {MAX_SHIFT}], got {d!r}")
    return int(d)


def sample_count(H: int, W: int, radius: int) -> int:
    """The samples of one frame's sums: (H - 1) row pairs times the W - 2R columns."""
    return (int(H) - 1) * (int(W) - 2 * int(radius))


def phase_sums(frames: Frames, idx: Sequence[int], radius: int) -> np.ndarray:
    """[len(idx), 2R + 1, 5] int64: entry [k][d + R] = (sum a, sum b, sum a^2, sum b^2, sum a*b) of
    frame idx[k] over every vertically adjacent row pair and the columns x in [R, W - R), a = the
    pair's odd row at x + d, b = its even row at x (sample_count of them for every d).  ``frames``:
    one device tensor or the slabs of one stack; ``idx``: global frame indices (any order,
    repeats allowed; an index outside the stack gives a zero row).  Each slab sums its own
    frames on its own device; the calls are queued on every device before a result is read."""
    parts = _slabs(frames)
    R = check_radius(radius)
    S = 2 * R + 1
    H, W = parts[0].shape[1:]
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    out = np.zeros((len(idx), S, 5), np.int64)
    fn = _lib.load().kcmc_bidi_phase_sums_u16
    pending, f0 = [], 0
    for p in parts:
        n = p.shape[0]
        rows = np.flatnonzero((idx >= f0) & (idx < f0 + n))
        dev = _device_of(p)
        if len(rows) or not pending:  # the first slab also without rows: it validates the arguments
            with torch.cuda.device(dev):
                o = torch.empty((len(rows), S, 5), dtype=torch.int64, device=dev)
                local = torch.from_numpy((idx[rows] - f0).astype(np.int32)).to(dev)
                _lib.check(fn(_ctx(dev).handle, _ptr(p), n, H, W, _ptr(local), len(rows), R, _ptr(o), _stream(dev)))
            pending.append((rows, o))
        f0 += n
    for rows, o in pending:
        if len(rows):
            out[rows] = o.cpu().numpy()
    return out


def sample_indices(n: int, k: int) -> List[int]:
    """The frames of a stack of ``n`` that are measured, at most ``k``: all of them when n <= k,
    else k of them spread evenly from the first to the last, (i (n - 1)) // (k - 1); k == 1 takes
    the middle frame n // 2."""
    n, k = int(n), int(k)
    if n < 0 or k < 1:
        raise ValueError(f"sample_indices: need n >= 0 and k >= 1, got {n}, {k}")
    if n <= k:
        return list(range(n))
    if k == 1:
        return [n // 2]
    return [(i * (n - 1)) // (k - 1) for i in range(k)]


def estimate_offset(sums: np.ndarray, n_samples: int, min_gain: float = 0.0) -> Tuple[int, np.ndarray, bool]:
    """(offset, correlations [2R + 1] float64, accepted) from phase_sums' [K, 2R + 1, 5] over K
    frames of ``n_samples`` samples each.

    The five sums are pooled over the frames in exact Python integers and r(d) is
    quality.pearson of the pooled sums over K n_samples samples.  The peak is the largest
    non-NaN r; ties go to the smaller |d|, then to the negative d.  offset = 0 with accepted =
    False when every r is NaN, when the peak sits on the window's border (|d| == R, R > 0: the
    search was saturated) or when the peak is not at 0 and r(peak) - r(0) <= min_gain (a NaN
    r(0) gains nothing to compare with and does not reject).  A peak at 0 is (0, r, True)."""
    sums = np.asarray(sums)
    if sums.ndim != 3 or sums.shape[2] != 5 or sums.shape[1] % 2 != 1:
        raise ValueError(f"sums must be [K, 2R + 1, 5], got {sums.shape}")
    K, S = sums.shape[:2]
    R = S // 2
    pooled = np.empty((S, 5), dtype=object)
    for j in range(S):
        for k in range(5):
            pooled[j, k] = sum(int(v) for v in sums[:, j, k])
    r = _q.pearson(pooled, K * int(n_samples))
    best = None
    for j in range(S):
        if math.isnan(r[j]):
            continue
        d = j - R
        key = (-float(r[j]), abs(d), d)
        if best is None or key < best:
            best = key
    if best is None:
        return 0, r, False
    d = best[2]
    if d == 0:
        return 0, r, True
    if abs(d) == R:
        return 0, r, False
    if not math.isnan(r[R]) and r[d + R] - r[R] <= float(min_gain):
        return 0, r, False
    return d, r, True


def shift_rows(frames: Frames, d: int, parity: int = 1, out: Optional[Frames] = None):
    """dst[f][y][x] = frames[f][y][clamp(x + d, 0, W - 1)] for the rows with (y & 1) == parity, the
    other rows as they are.  ``frames``: one device tensor [F, H, W] uint16 or the slabs of one
    stack; ``out``: None (new tensors), ``frames`` itself (in place: only the shifted rows are
    written) or tensors of the same shapes on the same devices that overlap nothing.  Works per
    slab, each under its own device; returns ``out`` in the form ``frames`` came in."""
    single = isinstance(frames, torch.Tensor)
    parts = _slabs(frames)
    d = check_shift(d)
    if parity not in (0, 1) or isinstance(parity, bool):
        raise ValueError(f"parity must be 0 or 1, got {parity!r}")
    if out is None:
        outs = [None] * len(parts)
    else:
        outs = [out] if isinstance(out, torch.Tensor) else list(out)
        if len(outs) != len(parts):
            raise ValueError("out: one tensor per slab")
    fn = _lib.load().kcmc_shift_rows_u16
    res = []
    for p, o in zip(parts, outs):
        dev = _device_of(p)
        with torch.cuda.device(dev):
            if o is None:
                o = torch.empty_like(p)
            _require(o, "out", torch.uint16, dev, 3)
            if o.shape != p.shape:
                raise ValueError(f"out: expected shape {tuple(p.shape)}, got {tuple(o.shape)}")
            F, H, W = p.shape
            if p.numel():
                _lib.check(fn(_ctx(dev).handle, _ptr(p), _ptr(o), F, H, W, int(parity), d, _stream(dev)))
        res.append(o)
    return res[0] if single else res
