"""What the passes over the pixels of an aligned uint16 stack share (quality, fallback, refine).
The stack is one device tensor [F, H, W] or its slabs on several devices; frame indices are
global, over the slabs in order."""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .multidevice import _on
from .pipeline import _runs
from .stages import _ctx, _device_of, _ptr, _require, _stream

Frames = Union[torch.Tensor, Sequence[torch.Tensor]]
Region = Tuple[int, int, int, int]


def _slabs(frames: Frames) -> List[torch.Tensor]:
    parts = [frames] if isinstance(frames, torch.Tensor) else list(frames)
    if not parts:
        raise ValueError("no frames")
    for p in parts:
        _require(p, "frames", torch.uint16, _device_of(p), 3)
        if p.shape[1:] != parts[0].shape[1:]:
            raise ValueError("the slabs of one stack must share H and W")
    return parts


def ref_tensor(ref, H: int, W: int) -> torch.Tensor:
    """The reference image as a tensor (on the device it is on), checked to be [H, W] uint16."""
    ref_t = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref))
    if ref_t.dtype != torch.uint16 or tuple(ref_t.shape) != (H, W):
        raise ValueError(f"ref must be [{H}, {W}] uint16")
    return ref_t


def parts_of(res) -> list:
    """The aligned slabs of a SlabResult (one tensor) or SplitResult (a list of them)."""
    return list(res.aligned) if isinstance(res.aligned, (list, tuple)) else [res.aligned]


def pass_parts(name: str, res) -> list:
    """parts_of(res) after the checks the fallback and the refinement open with (``name``: the pass)."""
    parts = parts_of(res)
    if parts[0].dim() != 3:
        raise NotImplementedError(f"the {name} supports grayscale stacks [F, H, W] only")
    if np.asarray(res.affines).shape[1:] != (2, 3):
        raise NotImplementedError(f"the {name} supports 2 x 3 maps only")
    return parts


def sample_mask(n_images: int, rate: int, skipped) -> np.ndarray:
    """[n_images] bool: every ``rate``-th frame that is not in ``skipped``."""
    gone = set(int(i) for i in skipped)
    sel = np.zeros(int(n_images), bool)
    sel[[i for i in range(0, int(n_images), int(rate)) if i not in gone]] = True
    return sel


def run_indexed(fn, parts, idx: np.ndarray, ref, rect: Region, trailing: tuple, tail: tuple):
    """The C entry point ``fn`` (kcmc_shift_search_u16, kcmc_gradient_sums_u16: ``trailing`` its
    arguments between the rectangle and the output; kcmc_tile_gradient_sums_u16: ``rect`` empty, the
    tile edges and their counts in ``trailing``) once per slab, over the frames ``idx`` (int64
    global indices, any order, repeats allowed) that lie in the slab.  Returns per call (rows, out):
    out the slab's device tensor [len(rows), *tail] int64, rows the positions in ``idx`` it answers;
    an index outside the stack is in no rows.  The calls are queued on every device before the
    caller reads a result; the first slab is called also without rows, which validates the arguments
    of an empty call.  A slab is passed as it is, 16-byte aligned or not (the kernels read either)."""
    H, W = parts[0].shape[1:]
    ref_t = ref_tensor(ref, H, W)
    pending, f0 = [], 0
    for p in parts:
        n = p.shape[0]
        rows = np.flatnonzero((idx >= f0) & (idx < f0 + n))
        dev = _device_of(p)
        if len(rows) or not pending:
            with torch.cuda.device(dev):
                out = torch.empty((len(rows), *tail), dtype=torch.int64, device=dev)
                local = torch.from_numpy((idx[rows] - f0).astype(np.int32)).to(dev)
                r = ref_t.to(dev).contiguous()
                _lib.check(fn(_ctx(dev).handle, _ptr(p), n, H, W, _ptr(local), len(rows), _ptr(r),
                              *(int(v) for v in rect), *trailing, _ptr(out), _stream(dev)))
            pending.append((rows, out))
        f0 += n
    return pending


def rewarp_runs(sources, parts, idxs, chunk=None):
    """(src, dst, f0, a, b) for the frames ``idxs`` (global indices): every maximal run [a, b) of them
    inside a slab, cut into pieces of at most ``chunk`` frames; src / dst the slab's source and
    aligned frames, f0 its first frame's global index.  Yields with dst's device current."""
    idxs = set(int(i) for i in idxs)
    f0 = 0
    for src, dst in zip(sources, parts):
        n = dst.shape[0]
        mine = np.array([f0 + j in idxs for j in range(n)], bool)
        with _on(dst):
            for a, b in _runs(mine):
                for a0 in range(a, b, chunk or b - a):
                    yield src, dst, f0, a0, min(b, a0 + (chunk or b - a))
        f0 += n
