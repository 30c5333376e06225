"""Staging of the warp's source box (warp.hip, mode 3): each thread owns one 16-byte chunk
column and every 14th box row, and loads through a buffer descriptor whose range check
supplies the zeros of BORDER_CONSTANT -- for rows above and below the frame, for rows below the
box, and (by an out-of-range first offset) for columns outside the frame or the box.

Every comparison is bit-exact against the CPU oracle's warpAffine.  The frame stacks live
inside larger buffers filled with 65535, at a 16-byte (not 32-byte) aligned offset, and the
three frames of a stack differ (dark / a few bright chunks / bright: the three blends), so a
tap that should read 0 but reads guard memory or the neighbouring frame changes the output.
The shapes are the smallest at which staging can go wrong: one tile, partial tiles in both
directions with two and three tile columns, and one frame height that takes 64-row tiles."""
import functools

import numpy as np
import pytest
import torch

import oracle
from kcmc_amd import stages, synthetic

pytestmark = pytest.mark.gpu

TILE_W, FAST_PITCH, FAST_ROWS = 128, 144, 71  # warp_tile.h kTileW; warp.hip kFastPitch, Fast<Cfg, 1>::kRows
MAX_PITCH, LDS_ELEMS, MAX_ROWS = 256, 10240, 72  # warp_tile.h kMaxPitch, kLdsElems, 8 * kRowPasses (BlockCfg)
GUARD, OFFSET = 4096, 8  # guard elements on each side; the stack starts 16 bytes past a 32-byte boundary

SHAPES = [(56, 128), (120, 136), (113, 264), (128, 136)]


def tile_h(H):
    return 64 if H % 64 == 0 and H % 56 != 0 else 56  # warp_tile.h use_tile64


def cv_round(v):
    return int(np.rint(v))


def source_box(Mi, xb, yb, H, W):
    """warp.hip source_box (affine_box of warp_tile.h, then box_plan) + the plan kernel's
    fast-path test, for the inverted map Mi: (mode, ax0, sy0, pitch, rows); mode 3 = fast staged path, 0 = general staged path,
    1 = every tap outside, 2 = direct gather."""
    th = tile_h(H)
    xl, yl = min(xb + TILE_W, W) - 1, min(yb + th, H) - 1
    m = [float(v) for v in Mi.reshape(6)]
    a0, a1 = cv_round(m[0] * xb * 1024), cv_round(m[0] * xl * 1024)
    b0, b1 = cv_round(m[3] * xb * 1024), cv_round(m[3] * xl * 1024)
    x0, x1 = cv_round((m[1] * yb + m[2]) * 1024) + 16, cv_round((m[1] * yl + m[2]) * 1024) + 16
    y0, y1 = cv_round((m[4] * yb + m[5]) * 1024) + 16, cv_round((m[4] * yl + m[5]) * 1024) + 16
    sx0, sx1 = (min(x0, x1) + min(a0, a1)) >> 10, ((max(x0, x1) + max(a0, a1)) >> 10) + 1
    sy0, sy1 = (min(y0, y1) + min(b0, b1)) >> 10, ((max(y0, y1) + max(b0, b1)) >> 10) + 1
    ax0 = (sx0 >> 3) << 3
    pitch = ((sx1 - ax0 + 1) + 7) & ~7
    rows = sy1 - sy0 + 1
    mode = 2
    if sx1 < 0 or sx0 > W - 1 or sy1 < 0 or sy0 > H - 1:
        mode = 1
    elif pitch <= MAX_PITCH and rows <= MAX_ROWS and pitch * rows <= LDS_ELEMS:
        mode = 0
    if W % 8 == 0 and mode == 0 and pitch <= FAST_PITCH and rows <= FAST_ROWS:
        mode = 3
    return mode, ax0, sy0, pitch, rows


def boxes(M, H, W):
    Mi = oracle.invert_affine(M)
    return [source_box(Mi, xb, yb, H, W) for yb in range(0, H, tile_h(H)) for xb in range(0, W, TILE_W)]


@functools.lru_cache(maxsize=None)
def frames(H, W):
    """Three frames: every value < 16384 (kDark); 13-bit noise with 3 % of the aligned 8-pixel
    groups bright (kMixed in most tiles); bright throughout (kBright)."""
    rng = np.random.default_rng(H * 1000 + W)
    dark = rng.integers(1, 16384, (H, W))
    mixed = rng.integers(1, 8192, (H, W))
    hot = np.repeat(rng.random((H, (W + 7) // 8)) < 0.03, 8, axis=1)[:, :W]
    mixed[hot] = rng.integers(30000, 65536, int(hot.sum()))
    bright = rng.integers(20000, 65536, (H, W))
    imgs = np.stack([dark, mixed, bright]).astype(np.uint16)
    imgs.setflags(write=False)
    return imgs


def warp_guarded(dev, imgs, Ms):
    """The library's warp of a stack that sits inside guard memory, into an output that does
    too; checks that no guard element of the output was written."""
    n = imgs.size
    lo, hi = GUARD + OFFSET, GUARD + OFFSET + n
    big = np.full(hi + GUARD, 65535, np.uint16)
    big[lo:hi] = imgs.reshape(-1)
    src_big = torch.from_numpy(big).to(dev)
    dst_big = torch.from_numpy(np.full(hi + GUARD, 65535, np.uint16)).to(dev)
    assert src_big.data_ptr() % 32 == 0 and dst_big.data_ptr() % 32 == 0
    src, dst = src_big[lo:hi].view(imgs.shape), dst_big[lo:hi].view(imgs.shape)
    assert src.data_ptr() % 32 == 16
    stages.warp_affine_u16(src, torch.from_numpy(np.ascontiguousarray(Ms)).to(dev), out=dst)
    res = dst_big.cpu().numpy()
    assert (res[:lo] == 65535).all() and (res[hi:] == 65535).all(), "the warp wrote outside its output"
    return res[lo:hi].reshape(imgs.shape)


def check(dev, H, W, M):
    imgs = frames(H, W)
    out = warp_guarded(dev, imgs, np.stack([M] * len(imgs)))
    for f, img in enumerate(imgs):
        ref = oracle.warp_affine_u16(img, M)
        bad = np.argwhere(out[f] != ref)
        assert bad.size == 0, (f, len(bad), bad[:4].tolist(), boxes(M, H, W))


def shift(dx, dy):
    """Forward map whose inverse puts output (y, x) on source (y + dy, x + dx)."""
    return np.array([[1.0, 0.0, -dx], [0.0, 1.0, -dy]])


# the identity, sub-pixel shifts, and shifts of 1-40 px that push the box across each of the
# four edges and each of the four corners of the frame
SHIFTS = [(0.0, 0.0), (0.3125, 0.59375), (-0.4, -0.7), (1.0, 0.0), (-1.25, 0.0), (0.0, 1.5), (0.0, -1.0),
          (17.3, 0.0), (-23.6, 0.0), (0.0, 31.2), (0.0, -40.0), (7.7, 9.4), (-12.1, 15.8), (38.9, -26.5),
          (-40.0, -33.3), (3.4, -2.1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_translations(dev, shape):
    H, W = shape
    modes = set()
    for dx, dy in SHIFTS:
        M = shift(dx, dy)
        tiles = {b[0] for b in boxes(M, H, W)}
        assert 3 in tiles  # the fast path stages a tile of every shift
        modes |= tiles
        check(dev, H, W, M)
    assert modes <= {1, 3}, modes  # (a narrow last tile column can be shifted off the frame: zeros)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_box_outside_the_frame(dev, shape):
    H, W = shape
    for dx, dy in [(W + 40.5, 0.0), (0.0, -(H + 77.25)), (-(W + 3.0), H + 3.0)]:
        M = shift(dx, dy)
        assert {b[0] for b in boxes(M, H, W)} == {1}
        check(dev, H, W, M)
    # a box whose last row / column alone is inside the frame, and whose first alone is
    for dx, dy in [(-(TILE_W - 0.5), 0.0), (W - 1.5, 0.0), (0.0, -(tile_h(H) - 0.5)), (0.0, H - 1.5)]:
        M = shift(dx, dy)
        assert 3 in {b[0] for b in boxes(M, H, W)}
        check(dev, H, W, M)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "%dx%d" % s)
def test_nan_map(dev, shape):
    """A frame without a model (NaN map) warps to zeros; its neighbours are warped as usual."""
    H, W = shape
    imgs = frames(H, W)
    M = synthetic.rigid(0.01, 1.3, -2.2)
    Ms = np.stack([M, np.full((2, 3), np.nan), M])
    out = warp_guarded(dev, imgs, Ms)
    assert not out[1].any()
    for f in (0, 2):
        assert np.array_equal(out[f], oracle.warp_affine_u16(imgs[f], M))


def zoom_rot(sx, sy, angle, tx, ty):
    M = synthetic.rigid(angle, tx, ty)
    M[:, 0] *= sx
    M[:, 1] *= sy
    return M


def sweep():
    """Rotations and zooms across the fast path's limits (box rows 71, box pitch 144)."""
    maps = []
    for a in np.arange(0.0, 0.1601, 0.004):
        maps += [zoom_rot(1.0, 1.0, a, 3.3, -2.6), zoom_rot(1.0, 1.0, -a, -1.7, 4.2)]
    for s in np.arange(1.0, 0.7999, -0.01):
        maps += [zoom_rot(s, 1.0, 0.0, 2.2, 1.1), zoom_rot(s, s, 0.01, 1.4, -0.8)]
    # 72 box rows fit the general path's 20 KB only at a pitch of 136: a zoom along y alone
    for s in np.arange(1.0, 0.7599, -0.005):
        maps.append(zoom_rot(1.0, s, 0.0, -0.6, 2.9))
    return maps


def limit_classes(M, H, W):
    cls = set()
    for mode, _, _, pitch, rows in boxes(M, H, W):
        if mode == 3 and rows == FAST_ROWS:
            cls.add("rows == kRows")
        if mode == 3 and pitch == FAST_PITCH:
            cls.add("pitch == 144")
        if mode == 0 and rows == FAST_ROWS + 1 and pitch <= FAST_PITCH:
            cls.add("rows just beyond")
        if mode == 0 and pitch == FAST_PITCH + 8 and rows <= FAST_ROWS:
            cls.add("pitch just beyond")
    return cls


ALL_CLASSES = {"rows == kRows", "pitch == 144", "rows just beyond", "pitch just beyond"}


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "%dx%d" % s)
def test_fast_path_limits(dev, shape):
    """Of the sweep, the first two maps that put some tile in each class (a box at the last
    row count / pitch the fast path takes, and one just beyond each, staged by the general
    path) and every fifth map besides."""
    H, W = shape
    chosen, count = [], {c: 0 for c in ALL_CLASSES}
    for i, M in enumerate(sweep()):
        new = [c for c in limit_classes(M, H, W) if count[c] < 2]
        for c in new:
            count[c] += 1
        if new or i % 5 == 0:
            chosen.append(M)
    assert all(v == 2 for v in count.values()), count
    for M in chosen:
        check(dev, H, W, M)


def test_width_not_a_multiple_of_8(dev):
    """W % 8 != 0: no tile takes the 16-byte staging (mode 3); the element-wise paths are as before."""
    H, W = 60, 132
    for M in [shift(0.0, 0.0), shift(5.3, -3.2), shift(-30.1, 20.6), synthetic.rigid(0.03, 2.3, -1.7)]:
        assert 3 not in {b[0] for b in boxes(M, H, W)}
        check(dev, H, W, M)
