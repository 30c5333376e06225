"""The detector's scale pyramid (csrc/resize.hip, kcmc_orb_detect_pyramid)
on the host: a numpy restatement of the pyramid around the per-level C oracle
(oracle.orb_detect), which tests/test_gpu_orb_pyramid.py runs the device against, and
host tests of (a) the restated resize at known answers, (b) orb.level_sizes /
level_quotas / level_to_base at the values DESIGN quotes, and (c) the reason the pyramid
exists: under a magnification of 1.44 the 8-level oracle chain (detect -> knn ->
ratio 0.75 -> similarity RANSAC) recovers the zoom and the 1-level chain does not.

Everything here restates the semantics from include/kcmc.h in Python integers and
doubles; nothing calls the code under test except where a test compares against it."""
import functools

import numpy as np
import pytest

import oracle
from kcmc_amd import orb
from test_orb_host import _texture_u8


# ------------------------------------------------------------------ the restatement
def axis_table(n, m):
    """Per destination index x of an axis resized n -> m: (first tap i, weight a of tap
    i + 1 in 1/2048), in Python integers."""
    idx, wgt = [], []
    for x in range(m):
        num, den = (2 * x + 1) * n - m, 2 * m
        i = num // den  # floor, also for num < 0
        a = ((num - i * den) * 2048 + m) // den
        if i < 0:
            i, a = 0, 0
        if i >= n - 1:
            i, a = n - 1, 0
        idx.append(i)
        wgt.append(a)
    return np.array(idx, np.int64), np.array(wgt, np.int64)


def resize_np(img, dh, dw):
    """The exact bilinear resize of one [H, W] u8 image (or a [F, H, W] stack)."""
    img = np.asarray(img)
    H, W = img.shape[-2:]
    iy, b = axis_table(H, dh)
    ix, a = axis_table(W, dw)
    iy1, ix1 = np.minimum(iy + 1, H - 1), np.minimum(ix + 1, W - 1)
    s = img.astype(np.int64)
    b, a = b[:, None], a[None, :]
    acc = (s[..., iy[:, None], ix[None, :]] * (2048 - b) * (2048 - a) + s[..., iy[:, None], ix1[None, :]] * (2048 - b) * a +
           s[..., iy1[:, None], ix[None, :]] * b * (2048 - a) + s[..., iy1[:, None], ix1[None, :]] * b * a)
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def sizes_np(H, W, n_levels, scale):
    return [(int(np.rint(H / scale ** l)), int(np.rint(W / scale ** l))) for l in range(n_levels)]


def quotas_np(n_features, n_levels, scale):
    f = 1.0 / scale
    d = n_features * (1.0 - f) / (1.0 - f ** n_levels)
    out = []
    for _ in range(n_levels - 1):
        out.append(int(np.rint(d)))
        d *= f
    return out + [max(n_features - sum(out), 0)]


def to_base(c, n_base, n_level):
    """One correctly rounded double division of two exact integers."""
    return np.array([float((2 * int(v) + 1) * n_base - n_level) / float(2 * n_level) for v in c], np.float64)


def pyramid_images(img, sizes):
    out = [np.ascontiguousarray(img)]
    for h, w in sizes[1:]:
        out.append(resize_np(out[-1], h, w))
    return out


def detect_pyramid_oracle(img, p, sizes=None, quotas=None):
    """(kp [n, 2] f64 in level-0 pixels, des [n, 32] u8, level [n] u8, per-level counts) of
    one image: oracle.orb_detect per level, level 0 first, packed."""
    H, W = img.shape
    sizes = sizes or sizes_np(H, W, p.n_levels, p.scale_factor)
    quotas = quotas or quotas_np(p.n_features, p.n_levels, p.scale_factor)
    kps, dess, lvls, counts = [], [], [], []
    imgs = pyramid_images(img, sizes)
    for l, ((h, w), q) in enumerate(zip(sizes, quotas)):
        if q == 0 or h < 2 * p.edge + 1 or w < 2 * p.edge + 1:
            counts.append(0)
            continue
        kp, des = oracle.orb_detect(imgs[l], n_features=q, threshold=p.fast_threshold, harris_k=p.harris_k, edge=p.edge,
                                    pattern=orb.rotated_patterns(), bin_cs=orb.bin_edges())
        kps.append(np.stack([to_base(kp[:, 0], W, w), to_base(kp[:, 1], H, h)], axis=1).reshape(-1, 2))
        dess.append(des)
        lvls.append(np.full(len(kp), l, np.uint8))
        counts.append(len(kp))
    if not kps:
        return np.zeros((0, 2)), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), counts
    return np.concatenate(kps), np.concatenate(dess), np.concatenate(lvls), counts


PYR_LAST_COUNT = {4: 24, 8: 24}  # cell -> the last level's count on pyramid_case_img(cell), of a quota of 31


def pyramid_case_img(cell=4, H=160, W=200, seed=21):
    return _texture_u8(np.random.default_rng(seed), H, W, cell=cell)


def thin_img():
    """40 rows: level 1 has 33, exactly 2 edge + 1 (one row of centres, which holds one
    keypoint at this seed); the levels from 2 on are too small."""
    return pyramid_case_img(4, 40, 200, seed=20)


# ------------------------------------------------------------------ the zoom scenario
ZOOM_H, ZOOM_W = 240, 320
ZOOM_SEED = 5


def _blur1(a):
    """Gaussian blur, sigma = 1, radius 4, edge replicated."""
    k = np.exp(-0.5 * np.arange(-4, 5) ** 2.0)
    k /= k.sum()
    for ax in (0, 1):
        pad = [(4, 4) if i == ax else (0, 0) for i in range(2)]
        p = np.pad(a, pad, mode="edge")
        a = sum(k[j] * np.take(p, np.arange(j, j + a.shape[ax]), axis=ax) for j in range(9))
    return a


@functools.lru_cache(maxsize=4)
def zoom_scene(seed=ZOOM_SEED, H=ZOOM_H, W=ZOOM_W):
    """Blocks of 6, 12 and 24 px, amplitude 60 each, added to 128, blurred (sigma 1);
    float64 [H, W]."""
    rng = np.random.default_rng(seed)
    s = np.full((H, W), 128.0)
    for cell in (6, 12, 24):
        lo = rng.uniform(-0.5, 0.5, (H // cell + 2, W // cell + 2))
        s += 60.0 * np.kron(lo, np.ones((cell, cell)))[:H, :W]
    return _blur1(s)


def zoom_frame(zoom, shift=(0.0, 0.0), seed=ZOOM_SEED, noise_seed=0):
    """The scene magnified by `zoom` about the frame centre and moved by shift = (dx, dy)
    (bilinear sampling, edge replicated), plus noise of sigma 2; float64 [H, W] in 0..255."""
    s = zoom_scene(seed)
    H, W = s.shape
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    xs = np.clip(cx + (np.arange(W) - shift[0] - cx) / zoom, 0, W - 1)
    ys = np.clip(cy + (np.arange(H) - shift[1] - cy) / zoom, 0, H - 1)
    x0, y0 = np.minimum(np.floor(xs).astype(int), W - 2), np.minimum(np.floor(ys).astype(int), H - 2)
    fx, fy = (xs - x0)[None, :], (ys - y0)[:, None]
    img = ((1 - fy) * ((1 - fx) * s[y0][:, x0] + fx * s[y0][:, x0 + 1]) +
           fy * ((1 - fx) * s[y0 + 1][:, x0] + fx * s[y0 + 1][:, x0 + 1]))
    img = img + np.random.default_rng([seed, noise_seed, 77]).normal(0, 2.0, img.shape)
    return np.clip(img, 0, 255)


def zoom_truth(zoom, shift=(0.0, 0.0), H=ZOOM_H, W=ZOOM_W):
    """The frame -> unzoomed-scene map of zoom_frame: (scale, tx, ty)."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return 1.0 / zoom, cx - (cx + shift[0]) / zoom, cy - (cy + shift[1]) / zoom


def oracle_chain(tpl_u8, frm_u8, p):
    """detect -> knn (template descriptors as queries) -> ratio 0.75 -> similarity RANSAC:
    (n_ratio_matches, n_inliers, params [2, 3] frame -> template)."""
    kt, dt, _, _ = detect_pyramid_oracle(tpl_u8, p)
    kf, df, _, _ = detect_pyramid_oracle(frm_u8, p)
    idx, dist = oracle.knn2_l2u8(dt, df)
    keep = dist[:, 0] < 0.75 * dist[:, 1]
    src, dst = kf[idx[keep, 0]], kt[keep]
    params, _, _, n_in = oracle.ransac_similarity(src, dst)
    return int(keep.sum()), n_in, params


# ------------------------------------------------------------------ resize
def test_resize_identity_and_exact_half():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 50)).astype(np.uint8)
    assert np.array_equal(resize_np(img, 37, 50), img)
    even = img[:36]
    s = even.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(resize_np(even, 18, 25), mean.astype(np.uint8))


@pytest.mark.parametrize("shape,dst", [((49, 131), (41, 109)), ((200, 260), (45, 56)), ((7, 5), (3, 2)),
                                       ((5, 7), (11, 16))])
def test_resize_constant_stays_constant(shape, dst):
    for v in (0, 1, 127, 255):
        assert (resize_np(np.full(shape, v, np.uint8), *dst) == v).all()


def test_resize_axis_table_at_the_size_limit():
    """num = (2x + 1) n - m reaches 2^33 at 65535 px: the table's ends stay in range and the
    weights in [0, 2048]."""
    n, m = 65535, 54613
    idx, wgt = axis_table(n, m)
    assert (2 * (m - 1) + 1) * n - m > 1 << 32
    assert idx[0] == 0 and 0 <= wgt[0] <= 2048
    assert idx[-1] == n - 2 and 0 < wgt[-1] <= 2048  # the last pair of taps, never past n - 1
    assert (np.diff(idx) >= 1).all() and idx.max() <= n - 1 and wgt.min() >= 0 and wgt.max() <= 2048
    up_i, up_a = axis_table(5, 16)  # upscaling: both ends clamp with weight 0
    assert up_i[0] == 0 and up_a[0] == 0 and up_i[-1] == 4 and up_a[-1] == 0


# ------------------------------------------------------------------ sizes, quotas, coordinates
SIZES_160x200 = [(160, 200), (133, 167), (111, 139), (93, 116), (77, 96), (64, 80), (54, 67), (45, 56)]
QUOTAS_500 = [109, 90, 75, 63, 52, 44, 36, 31]


def test_level_sizes_and_quotas():
    assert orb.level_sizes(160, 200, 8, 1.2) == SIZES_160x200 == sizes_np(160, 200, 8, 1.2)
    assert orb.level_quotas(500, 8, 1.2) == QUOTAS_500 == quotas_np(500, 8, 1.2)
    few = orb.level_quotas(5, 8, 1.2)
    assert few == quotas_np(5, 8, 1.2) and sum(few) == 5 and 0 in few and min(few) == 0
    assert orb.level_quotas(500, 1, 1.2) == [500] and orb.level_sizes(33, 47, 1, 1.2) == [(33, 47)]
    for n, L, s in ((500, 3, 1.5), (1, 8, 1.2), (0, 4, 1.2), (77, 2, 2.0)):
        q = orb.level_quotas(n, L, s)
        assert q == quotas_np(n, L, s) and len(q) == L and min(q) >= 0 and sum(q) == n
    assert orb.level_sizes(240, 320, 3, 1.5) == sizes_np(240, 320, 3, 1.5) == [(240, 320), (160, 213), (107, 142)]
    p = orb.OrbParams()
    assert p.n_levels == 1 and p.scale_factor == 1.2
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(scale_factor=1.0), dict(scale_factor=0.5)):
        kw = dict(n_levels=2, scale_factor=1.2)
        kw.update(bad)
        with pytest.raises(ValueError):
            orb.level_sizes(100, 100, **kw)
        with pytest.raises(ValueError):
            orb.level_quotas(100, **kw)


def test_coordinate_map():
    x = np.arange(200)
    assert np.array_equal(orb.level_to_base(x, 200, 200), x.astype(np.float64))  # level 0: exactly x
    # level 1 of a 200-wide frame (167 px): x_l = 10 -> (21 * 200 - 167) / 334 = 4033 / 334
    assert orb.level_to_base(10, 200, 167) == 4033.0 / 334.0
    assert np.array_equal(orb.level_to_base(np.arange(167), 200, 167), to_base(np.arange(167), 200, 167))
    # the map is the resize's own: pixel x_l samples level 0 at i + a / 2048 up to the weight's rounding
    idx, wgt = axis_table(200, 167)
    assert np.abs(orb.level_to_base(np.arange(167), 200, 167) - (idx + wgt / 2048.0)).max() <= 0.5 / 2048 + 1e-12
    # the centre maps to the centre: no drift from the rounded level size
    assert orb.level_to_base(83, 200, 167) == 99.5


def test_pyramid_oracle_packs_and_underfills():
    """The GPU cases' premises: on 160x200 the last level leaves part of its quota unused
    (PYR_LAST_COUNT of 31), so the packed rows end before n_features; a 40-row frame
    detects on levels 0 and 1 only."""
    p = orb.OrbParams(n_levels=8)
    for cell, last in PYR_LAST_COUNT.items():
        img = pyramid_case_img(cell)
        kp, des, lvl, counts = detect_pyramid_oracle(img, p)
        assert counts[:7] == QUOTAS_500[:7] and counts[7] == last < QUOTAS_500[7], (cell, counts)
        assert len(kp) == sum(counts) == len(des) == len(lvl) and (np.diff(lvl.astype(int)) >= 0).all()
        assert kp[:, 0].min() >= 16 and kp[:, 0].max() <= 200 - 17 + 1 and kp[:109, 0].tolist() == np.rint(kp[:109, 0]).tolist()
    counts = detect_pyramid_oracle(thin_img(), p)[3]
    assert sizes_np(40, 200, 8, 1.2)[1:3] == [(33, 167), (28, 139)]
    assert counts[0] > 0 and counts[1] == 1 and counts[2:] == [0] * 6, counts


# ------------------------------------------------------------------ effectiveness
def test_pyramid_recovers_a_zoom_the_single_level_loses():
    """Zoom 1.44 about the centre, 500 features: 8 levels give >= 40 RANSAC inliers, the
    scale within 0.5 % and the translation within 1 px; one level gives < 8 inliers.
    (Measured over seeds: 54-84 inliers, <= 0.13 %, <= 0.37 px against 2-3 inliers; the
    bounds carry about 3x margin.)"""
    tpl = zoom_frame(1.0, noise_seed=0).astype(np.uint8)
    frm = zoom_frame(1.44, noise_seed=1).astype(np.uint8)
    scale, tx, ty = zoom_truth(1.44)
    n_ratio, n_in, params = oracle_chain(tpl, frm, orb.OrbParams(n_levels=8))
    got = np.hypot(params[0, 0], params[1, 0])
    print("8 levels:", n_ratio, n_in, got / scale - 1, params[0, 2] - tx, params[1, 2] - ty)
    assert n_in >= 40
    assert abs(got / scale - 1) <= 0.005
    assert np.hypot(params[0, 2] - tx, params[1, 2] - ty) <= 1.0
    n_ratio1, n_in1, _ = oracle_chain(tpl, frm, orb.OrbParams(n_levels=1))
    print("1 level:", n_ratio1, n_in1)
    assert n_in1 < 8
