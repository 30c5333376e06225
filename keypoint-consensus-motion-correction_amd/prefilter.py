"""Box band-pass prefilter in front of keypoint detection (csrc/band_filter.hip).

One-photon, miniscope and widefield stacks carry their cells as a few hundred grey levels on a
smooth background of tens of thousands: after the max-scaling to uint8 the cells are a level or
two high and the detector sees the vignette only.  Shot-noise-limited two-photon frames want a
small smoothing before detection.  Both are served by a copy of the stack that only the
detection reads (VideoAligner.DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS): the rounded mean
over a (2s + 1)^2 box minus the rounded mean over a (2r + 1)^2 box, both clipped to the image,
floored at 0.  Build-defined: the reference has no such mode; the semantics are written down in
include/kcmc.h and DESIGN.md (p1) and restated in numpy in tests/test_prefilter_host.py.

  check_radii    the rules of the two radii
  box_bandpass   kcmc_box_bandpass_u16: the filtered copy of a stack or of its slabs
  launch_plan    kcmc_box_bandpass_plan: the kernel's strips and row chunks (for tests at its seams)

Grayscale stacks [F, H, W].
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._intensity import Frames, _slabs
from .stages import _ctx, _device_of, _ptr, _require, _stream

MAX_SMOOTH = 4
MAX_BACKGROUND = 32


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_radii(smooth, background) -> Tuple[int, int]:
    """(s, r) as ints: s in [0, 4]; r either 0 or in [s + 1, 32]; not both 0."""
    if not (_is_int(smooth) and 0 <= int(smooth) <= MAX_SMOOTH):
        raise ValueError(f"the smoothing radius must be an integer in [0, {MAX_SMOOTH}], got {smooth!r}")
    if not (_is_int(background) and 0 <= int(background) <= MAX_BACKGROUND):
        raise ValueError(f"the background radius must be 0 or an integer in [1, {MAX_BACKGROUND}], got "
                         f"{background!r}")
    s, r = int(smooth), int(background)
    if s == 0 and r == 0:
        raise ValueError("the smoothing and the background radius are both 0: no filter")
    if 0 < r <= s:
        raise ValueError(f"the background radius must be 0 or exceed the smoothing radius, got {r} <= {s}")
    return s, r


def launch_plan(n_frames: int, H: int, W: int, smooth: int, background: int) -> Tuple[int, int, int, int]:
    """kcmc_box_bandpass_plan: how the kernel cuts that call -- (output columns of one workgroup's
    strip, strips per frame, row chunks per frame, rows per chunk).  Asked of the library, not
    restated here; needs no GPU."""
    s, r = check_radii(smooth, background)
    plan = (ctypes.c_int * 4)()
    _lib.check(_lib.load().kcmc_box_bandpass_plan(int(n_frames), int(H), int(W), s, r, plan))
    return tuple(int(v) for v in plan)


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def box_bandpass(frames: Frames, smooth: int, background: int, out: Optional[Frames] = None):
    """dst[f][y][x] = max(m_s - m_r, 0) of frames[f] (m_rho: the rounded mean over the box of radius rho
    clipped to the image, m_r = 0 with background = 0; include/kcmc.h).  ``frames``: one device
    tensor [F, H, W] uint16 or the slabs of one stack; ``out``: None (new tensors) or tensors of the
    same shapes on the same devices that overlap no input.  Works per slab, each under its own
    device, every launch queued before anything is read; returns ``out`` in the form ``frames``
    came in."""
    single = isinstance(frames, torch.Tensor)
    parts = _slabs(frames)
    s, r = check_radii(smooth, background)
    if out is None:
        outs = [None] * len(parts)
    else:
        outs = [out] if isinstance(out, torch.Tensor) else list(out)
        if len(outs) != len(parts):
            raise ValueError("out: one tensor per slab")
        for o in outs:
            _require(o, "out", torch.uint16, _device_of(o), 3)
            for p in parts:
                if o.numel() and p.numel() and o.device == p.device and _overlap(o, p):
                    raise ValueError("out overlaps the input (a neighbourhood filter cannot run in place)")
    fn = _lib.load().kcmc_box_bandpass_u16
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
                _lib.check(fn(_ctx(dev).handle, _ptr(p), _ptr(o), F, H, W, s, r, _stream(dev)))
        res.append(o)
    return res[0] if single else res
