"""The warp's certified integer blend: of the pixels whose exact blend sum S = sum v_k K_k is
>= 2^24 only those with S mod 1024 within kTieWindow of 512 are re-blended with OpenCV's
float formula (warp.hip near_tie; proof in DESIGN 4 K3).  Every comparison is bit-exact
against the CPU oracle; the census tests first prove on the host, from the exact integer
sums, that the data holds pixels inside the window, pixels where the float formula differs
from rint(S / 1024), and bright pixels outside the window -- and fail if a class is missing."""
import functools

import numpy as np
import pytest
import torch

import oracle
from kcmc_amd import stages, synthetic

pytestmark = pytest.mark.gpu

K_TIE_WINDOW = 16  # warp.hip kTieWindow
H0, W0 = 60, 136   # one full and one partial 128-px tile column, one full and one partial 56-row tile row


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cached inputs are read-only


def cv_round(v):
    return int(np.rint(v))  # round half to even, as cvRound


def shift_map(dx, fx, dy, fy):
    """Translation-only forward map whose inverse puts output (y, x) on source
    (y + dy + fy/32, x + dx + fx/32): every pixel of the frame has the fractions (fx, fy)."""
    return np.array([[1.0, 0.0, -(dx + fx / 32.0)], [0.0, 1.0, -(dy + fy / 32.0)]])


def fixed_point_origin(M):
    """(sx0, fx, sy0, fy) of a translation-only map, the way warpAffine derives them: the
    inverted map, X0 = cvRound(M2 * 1024) + 16, X = (X0 + 1024 x) >> 5, sx = X >> 5, fx = X & 31."""
    Mi = oracle.invert_affine(M)
    assert Mi[0, 0] == 1.0 and Mi[1, 1] == 1.0 and Mi[0, 1] == 0.0 and Mi[1, 0] == 0.0
    X0 = (cv_round(Mi[0, 2] * 1024) + 16) >> 5
    Y0 = (cv_round(Mi[1, 2] * 1024) + 16) >> 5
    return X0 >> 5, X0 & 31, Y0 >> 5, Y0 & 31


def exact_sums(img, M):
    """S = sum v_k K_k per output pixel (and channel) in exact integers, zero border."""
    sx0, fx, sy0, fy = fixed_point_origin(M)
    H, W = img.shape[:2]
    pad = 8
    assert max(abs(sx0), abs(sy0)) + 2 <= pad
    big = np.zeros((H + 2 * pad, W + 2 * pad) + img.shape[2:], np.int64)
    big[pad:pad + H, pad:pad + W] = img

    def tap(oy, ox):
        return big[pad + sy0 + oy:pad + sy0 + oy + H, pad + sx0 + ox:pad + sx0 + ox + W]

    ax, ay = 32 - fx, 32 - fy
    return tap(0, 0) * (ay * ax) + tap(0, 1) * (ay * fx) + tap(1, 0) * (fy * ax) + tap(1, 1) * (fy * fx)


def tile_blend(img, M, xb=0, yb=0, tile_h=56):
    """The blend the one-channel fast path picks for the tile at (xb, yb) under a
    translation-only map: the tile's staged box (source_box in warp.hip, affine_box in warp_tile.h) and its bright
    16-byte chunks against kBrightShare = 20."""
    sx0, _, sy0, _ = fixed_point_origin(M)
    H, W = img.shape
    xl, yl = min(xb + 128, W) - 1, min(yb + tile_h, H) - 1
    c0, c1, r0, r1 = sx0 + xb, sx0 + xl + 1, sy0 + yb, sy0 + yl + 1
    ax0 = (c0 >> 3) << 3
    cpr, rows = (((c1 - ax0 + 1) + 7) & ~7) >> 3, r1 - r0 + 1
    bright = 0
    for r in range(max(r0, 0), min(r1, H - 1) + 1):
        for c in range(cpr):
            gx = ax0 + 8 * c
            bright += int(0 <= gx < W and (img[r, gx:gx + 8] >= 16384).any())
    total = rows * cpr
    return "dark" if bright == 0 else "mixed" if bright * 20 <= total else "bright"


def in_window(S, extra=0):
    return (S >= 1 << 24) & (np.abs((S & 1023) - 512) <= K_TIE_WINDOW + extra)


def round_exact(S):
    return np.rint(S / 1024.0).astype(np.int64)  # S < 2^26: the fp64 quotient is exact


@functools.lru_cache(maxsize=None)
def mixed_frames(F, H, W, C=0, seed=5):
    """Data in 14000..16383 with 4.3 % of the aligned 8-pixel groups in 40000..65535: most
    tiles hold bright 16-byte chunks, but under a twentieth of the staged box (kMixed: the
    integer blend, and the float blend for rows with a sum near a tie).  Whole groups,
    because the kernel counts bright chunks: isolated bright pixels at that chunk count would
    give too few bright sums for the census at this frame size; and a high dark level, so
    that every output a bright pixel touches has S >= 2^24."""
    rng = np.random.default_rng(seed)
    shape = (F, H, W) + ((C,) if C else ())
    imgs = rng.integers(14000, 16384, shape)
    hot = np.repeat(rng.random((F, H, W // 8)) < 0.043, 8, axis=2)
    imgs[hot] = rng.integers(40000, 65536, imgs[hot].shape)
    imgs = imgs.astype(np.uint16)
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def bright_frames(F, H, W, C=0, seed=6):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(20000, 65536, (F, H, W) + ((C,) if C else ())).astype(np.uint16)
    imgs.setflags(write=False)
    return imgs


def census_maps(F, seed):
    rng = np.random.default_rng(seed)
    # odd fractions in 9..23: all four weights K_k are odd (the float products of 16-bit taps
    # need rounding) and at least 0.08 (a bright tap lifts all four of its outputs)
    return np.stack([shift_map(int(rng.integers(-3, 4)), int(rng.integers(4, 12)) * 2 + 1,
                               int(rng.integers(-3, 4)), int(rng.integers(4, 12)) * 2 + 1) for _ in range(F)])


def census(imgs, Ms):
    """(pixels with S >= 2^24 inside the window, pixels where the oracle differs from
    rint(S / 1024), pixels with S >= 2^24 outside the window), and the oracle's frames."""
    n_in = n_diff = n_out = 0
    refs = []
    for img, M in zip(imgs, Ms):
        S = exact_sums(img, M)
        ref = oracle.warp_affine_u16(img, M)
        win = in_window(S)
        diff = ref.astype(np.int64) != round_exact(S)
        assert not (diff & ~win).any(), "the float blend differs from rint(S / 1024) outside the window"
        n_in += int(win.sum())
        n_diff += int(diff.sum())
        n_out += int(((S >= 1 << 24) & ~win).sum())
        refs.append(ref)
    return (n_in, n_diff, n_out), refs


def check_census(counts):
    n_in, n_diff, n_out = counts
    print("census: in window", n_in, "oracle != rint(S/1024)", n_diff, "bright outside the window", n_out)
    assert n_in >= 200, counts
    assert n_diff >= 5, counts
    assert n_out >= 1000, counts


@pytest.mark.parametrize("data", ["mixed", "bright"])
def test_census_translation_maps(dev, data):
    """Constant (fx, fy) per frame, so the host knows every pixel's exact sum: the data holds
    every class of pixel, and the kernel matches the oracle on all of them."""
    F = 8
    imgs = mixed_frames(F, H0, W0) if data == "mixed" else bright_frames(F, H0, W0)
    Ms = census_maps(F, seed=11)
    counts, refs = census(imgs, Ms)
    check_census(counts)
    blends = [tile_blend(imgs[f], Ms[f]) for f in range(F)]  # each frame's full tile
    if data == "mixed":
        assert blends.count("mixed") >= 5, blends
    else:
        assert blends == ["bright"] * F
    out = stages.warp_affine_u16(_t(imgs, dev), _t(Ms, dev)).cpu().numpy()
    for f in range(F):
        assert np.array_equal(out[f], refs[f]), f


EDGE = K_TIE_WINDOW + 4


HE, WE = 168, 264  # window-edge frame: 3 x 3 tiles, the last of each partial


@functools.lru_cache(maxsize=None)
def window_edge_frame(H=HE, W=WE, row_step=8, col_step=64):
    """One frame of 14-bit noise with sparse 2 x 2 bright blocks (every 8th row pair, every
    8th 16-byte chunk: under a twentieth of a staged box, so the full tiles are kMixed), each
    block the four taps of one output pixel under the map
    (dx, dy) = (0, 0), (fx, fy) = (13, 7), chosen so that S >= 2^24 and S mod 1024 takes
    every value in 512 +- (kTieWindow + 4), on even and odd multiples of 1024."""
    fx, fy = 13, 7
    Kw = np.array([(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx], np.int64)
    rng = np.random.default_rng(3)
    cand = rng.integers(20000, 65536, (400000, 4))
    Sc = cand @ Kw
    assert (Sc >= 1 << 24).all()
    img = rng.integers(0, 16384, (H, W))
    slots = [(y, x) for y in range(0, H - 1, row_step) for x in range(0, W - 1, col_step)]
    targets = [512 + d for d in range(-EDGE, EDGE + 1)]
    for n, (y, x) in enumerate(slots):
        r = targets[n % len(targets)]
        parity = (n // len(targets)) & 1  # ties round to even: both parities of S >> 10
        pick = np.flatnonzero(((Sc & 1023) == r) & (((Sc >> 10) & 1) == parity))
        assert pick.size, (r, parity)
        t = cand[pick[n % pick.size]]
        img[y, x], img[y, x + 1], img[y + 1, x], img[y + 1, x + 1] = t
    img = img.astype(np.uint16)
    img.setflags(write=False)
    return img, shift_map(0, fx, 0, fy)


def test_window_edges(dev):
    img, M = window_edge_frame()
    S = exact_sums(img, M)
    bright = S >= 1 << 24
    res = set(zip(((S[bright] & 1023) - 512).tolist(), ((S[bright] >> 10) & 1).tolist()))
    missing = [(d, par) for d in range(-EDGE, EDGE + 1) for par in (0, 1) if (d, par) not in res]
    assert not missing, missing
    blends = [tile_blend(img, M, xb, yb) for yb in (0, 56) for xb in (0, 128)]  # the full tiles
    assert blends == ["mixed"] * 4, blends
    ref = oracle.warp_affine_u16(img, M)
    assert not ((ref.astype(np.int64) != round_exact(S)) & ~in_window(S)).any()
    out = stages.warp_affine_u16(_t(img[None], dev), _t(M[None], dev)).cpu().numpy()
    assert np.array_equal(out[0], ref)
    # the same taps through the perspective kernel's blend
    Mp = np.concatenate([M, [[0.0, 0.0, 1.0]]])
    outp = stages.warp_perspective_u16(_t(img[None], dev), _t(Mp[None], dev)).cpu().numpy()
    assert np.array_equal(outp[0], oracle.warp_perspective_u16(img, Mp))


def test_many_rows_made_again(dev):
    """A tile that stays kMixed (38 bright chunks of its 986) while over a quarter of its rows
    hold a pixel inside the window -- every wave leaves several rows to its float loop -- beside
    a tile column with no bright value at all."""
    img, M = window_edge_frame(H0, W0, 3, W0)
    assert tile_blend(img, M) == "mixed" and tile_blend(img, M, xb=128) == "dark"
    rows = in_window(exact_sums(img, M))[:56, :128].any(1)
    assert rows.sum() >= 15 and min(rows[w::4].sum() for w in range(4)) >= 3, rows.nonzero()
    out = stages.warp_affine_u16(_t(img[None], dev), _t(M[None], dev)).cpu().numpy()
    assert np.array_equal(out[0], oracle.warp_affine_u16(img, M))


def zoom(s, angle, tx, ty):
    M = synthetic.rigid(angle, tx, ty)
    M[:, :2] *= s
    return M


# near-identity maps (fast path), maps that push the source box over the frame's edges (taps
# read zeros), and an anisotropic zoom-out whose 128-px tile reads a 160-px wide box: wider
# than the fast path's 144-px pitch, so the general staged path
NEAR_MAPS = [synthetic.rigid(0.03, 2.3, -1.7), synthetic.rigid(-0.03, -3.6, 2.2), zoom(1.05, 0.0, -3.1, -1.4),
             zoom(1.05, 0.01, 1.2, 0.6), synthetic.rigid(0.02, 9.4, 7.7), synthetic.rigid(-0.02, -11.3, -6.1),
             np.array([[0.8, 0.0, 3.3], [0.0, 1.0, 1.7]])]


def _check_affine(dev, imgs, Ms):
    out = stages.warp_affine_u16(_t(imgs, dev), _t(np.stack(Ms), dev)).cpu().numpy()
    for f, M in enumerate(Ms):
        assert np.array_equal(out[f], oracle.warp_affine_u16(imgs[f], M)), f


@pytest.mark.parametrize("data", ["mixed", "bright"])
@pytest.mark.parametrize("H", [60, 64, 128])
def test_rotated_and_zoomed_maps(dev, data, H):
    """56-row tiles (H = 60) and the 64-row tile configuration (H = 64, 128)."""
    F = len(NEAR_MAPS)
    imgs = mixed_frames(F, H, W0) if data == "mixed" else bright_frames(F, H, W0)
    _check_affine(dev, imgs, NEAR_MAPS)


@pytest.mark.parametrize("data", ["mixed", "bright"])
@pytest.mark.parametrize("C", [3, 4])
def test_rotated_and_zoomed_maps_multichannel(dev, data, C):
    F = len(NEAR_MAPS)
    imgs = mixed_frames(F, 48, W0, C) if data == "mixed" else bright_frames(F, 48, W0, C)
    _check_affine(dev, imgs, NEAR_MAPS)


@pytest.mark.parametrize("C", [3, 4])
def test_multichannel_census(dev, C):
    """Translation maps on C = 3 / 4: the planar fast path's per-row decision is taken over
    every channel's sums."""
    F = 8
    imgs = mixed_frames(F, 48, W0, C, seed=9)
    Ms = census_maps(F, seed=13)
    counts, refs = census(imgs, Ms)
    n_in, _, n_out = counts
    assert n_in >= 200 and n_out >= 1000, counts
    out = stages.warp_affine_u16(_t(imgs, dev), _t(Ms, dev)).cpu().numpy()
    for f in range(F):
        assert np.array_equal(out[f], refs[f]), f


@pytest.mark.parametrize("data", ["mixed", "bright"])
@pytest.mark.parametrize("C", [0, 3])
def test_perspective(dev, data, C):
    Ms = [np.array([[1.0, 0.01, 2.3], [-0.01, 1.0, -1.6], [1e-5, 2e-5, 1.0]]),
          np.array([[1.02, -0.02, -4.4], [0.015, 0.99, 3.2], [-2e-5, 1e-5, 1.0]])]
    imgs = mixed_frames(2, H0, W0, C) if data == "mixed" else bright_frames(2, H0, W0, C)
    out = stages.warp_perspective_u16(_t(imgs, dev), _t(np.stack(Ms), dev)).cpu().numpy()
    for f, M in enumerate(Ms):
        assert np.array_equal(out[f], oracle.warp_perspective_u16(imgs[f], M)), f
