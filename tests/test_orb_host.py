"""Edge cases of the build's ORB-style detector (f1, csrc/orb.hip): the case generators
that tests/test_gpu_orb.py runs on the device, and host tests that (a) pin the C oracle
to the pure-Python restatement of tests/test_oracle_orb.py at these cases and (b) prove
from oracle data that each case reaches the branch it is named for -- NMS ties across
tile and region seams, moments exactly on a bin edge, negative Harris keys, a select cut
inside a tie group longer than one 256-candidate chunk, more than 100 candidates in one
tile, the smallest frame, every staging width.

A case is (name, imgs [F, H, W] u8, OrbParams).  Every image is seeded; the budgets and
the mixed-sign harris_k below were chosen on the CPU from oracle data and the host tests
assert the property each was chosen for, so a change of the generators cannot silently
turn a case into a plain one."""
import functools

import numpy as np
import pytest

import oracle
from kcmc_amd import orb
from test_oracle_orb import (bin_py, candidates_py, describe_py, fast_score_py, harris_py, moments_py, score_map_py,
                             select_py)

UNLIMITED = 1 << 16  # a budget no frame of these sizes reaches


def _texture_u8(rng, H, W, cell=4, noise=12):
    """Random block texture (the one of tests/test_gpu_models.py)."""
    lo = rng.integers(0, 256, (H // cell + 2, W // cell + 2)).astype(np.float64)
    img = np.kron(lo, np.ones((cell, cell)))[:H, :W] + rng.normal(0, noise, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


def _P(**kw):
    return orb.OrbParams(**kw)


# ------------------------------------------------------------------ generators
def single_pixel_img(H=33, W=33):
    img = np.zeros((H, W), np.uint8)
    img[16, 16] = 255
    return img


# companion offsets (dx, dy): the moments (m10, m01) = 90 (dx, dy) point along 0, 45, ... 315
# degrees, exactly the edges between bins 31|0, 3|4, ... 27|28
COMPASS_OFFSETS = [(7, 0), (7, 7), (0, 7), (-7, 7), (-7, 0), (-7, -7), (0, -7), (7, -7)]
COMPASS_DOTS = [(30 + 36 * i, 40) for i in range(8)]  # (x, y)


def compass_img():
    img = np.zeros((80, 330), np.uint8)
    for (x, y), (dx, dy) in zip(COMPASS_DOTS, COMPASS_OFFSETS):
        img[y, x] = 255
        img[y + dy, x + dx] = 90
    return img


# (y, x, size) of the squares of value 200: each straddles a 64x16 tile seam (x = 63|64,
# y = 15|16 mod 16) and / or a workgroup-region seam (y = 31|32 mod 32)
SEAM_SQUARES = [(31, 63, 2), (31, 100, 3), (40, 63, 2), (47, 63, 3), (31, 20, 2), (63, 63, 2)]


def seams_img():
    img = np.zeros((80, 160), np.uint8)
    for y, x, n in SEAM_SQUARES:
        img[y:y + n, x:x + n] = 200
    return img


GEOMETRY_SHAPES = ([(49, W) for W in (33, 34, 35, 36, 63, 64, 65, 67, 128, 129, 131, 192)] +
                   [(H, W) for H in (33, 34, 47, 48, 49, 64, 65) for W in (67, 128) if H != 49])
# the first seed (counting from 0) for which both frames hold a keypoint inside the margin
GEOMETRY_SEED = {(49, 34): 1, (33, 67): 3}


def geometry_imgs(H, W):
    rng = np.random.default_rng(1000 * H + W + 100000 * GEOMETRY_SEED.get((H, W), 0))
    return np.stack([_texture_u8(rng, H, W) for _ in range(2)])


EDGES = (16, 17, 24, 40, 59, 60)


def edges_img():
    return _texture_u8(np.random.default_rng(11), 120, 200)


THRESHOLDS = (0, 1, 100, 254, 255)
HARRIS_KS = (0.0, 0.04, 0.25)
HARRIS_K_MIXED = 0.2   # both signs occur (test_harris_sign_cases)
HARRIS_N_POS = 110     # the number of positive responses at HARRIS_K_MIXED


def binary_blocks_img():
    rng = np.random.default_rng(12)
    lo = rng.integers(0, 2, (96 // 4, 131 // 4 + 1)).astype(np.uint8) * 255
    return np.ascontiguousarray(np.kron(lo, np.ones((4, 4), np.uint8))[:96, :131])


def ties_img():
    block = np.random.default_rng(13).integers(0, 256, (8, 8)).astype(np.uint8)
    return np.ascontiguousarray(np.tile(block, (25, 38))[:200, :304])


TIES_TOTAL = 4284        # candidates of ties_img: 6 Harris values, 714 candidates each (test_ties_cases)
TIES_CUTS = (400, 1114)  # budgets whose cut falls inside a 714-tie group with 400 ties taken (> one chunk)


def dense_img():
    return np.random.default_rng(14).integers(0, 256, (96, 192)).astype(np.uint8)


DENSE_THRESHOLDS = (5, 20)


@functools.lru_cache(maxsize=1)
def cases():
    out = [("single_pixel", single_pixel_img()[None], _P()),
           ("single_pixel/32x100", np.zeros((1, 32, 100), np.uint8), _P()),
           ("single_pixel/100x32", np.zeros((1, 100, 32), np.uint8), _P()),
           ("single_pixel/32x32", np.zeros((1, 32, 32), np.uint8), _P()),
           ("compass", compass_img()[None], _P()),
           ("seams", seams_img()[None], _P())]
    for name, imgs, _ in out[1:4]:
        imgs[0, 16, 16] = 255  # the dot that a 33x33 frame keeps; here no pixel is admissible
    for H, W in GEOMETRY_SHAPES:
        out.append((f"geometry/{H}x{W}", geometry_imgs(H, W), _P()))
    e = edges_img()[None]
    out += [(f"edges/{edge}", e, _P(edge=edge)) for edge in EDGES]
    b = binary_blocks_img()[None]
    out += [(f"thresholds/{t}", b, _P(fast_threshold=t)) for t in THRESHOLDS]
    out += [(f"harris_sign/k={k}", b, _P(harris_k=k)) for k in HARRIS_KS]
    out += [(f"harris_sign/mixed/n={HARRIS_N_POS + d}", b, _P(harris_k=HARRIS_K_MIXED, n_features=HARRIS_N_POS + d))
            for d in (-1, 0, 1)]
    t = ties_img()[None]
    out += [(f"ties/n={n}", t, _P(n_features=n)) for n in (1, *TIES_CUTS, TIES_TOTAL - 1, TIES_TOTAL, TIES_TOTAL + 1)]
    d = dense_img()[None]
    out += [(f"dense/t={t}", d, _P(fast_threshold=t, n_features=UNLIMITED)) for t in DENSE_THRESHOLDS]
    return out


CASE_NAMES = [c[0] for c in cases()]
EMPTY_CASES = {"single_pixel/32x100", "single_pixel/100x32", "single_pixel/32x32", "edges/60", "thresholds/255"}


def case(name):
    return next(c for c in cases() if c[0] == name)


# ------------------------------------------------------------------ oracle access
def detect_oracle(img, p):
    return oracle.orb_detect(img, n_features=p.n_features, threshold=p.fast_threshold, harris_k=p.harris_k, edge=p.edge,
                             pattern=orb.rotated_patterns(), bin_cs=orb.bin_edges())


def oracle_bin(img, x, y):
    a = np.ascontiguousarray(img)
    return oracle.lib().kcmc_oracle_orientation_bin(a.ctypes.data_as(oracle.ctypes.c_void_p), a.shape[1], int(x), int(y),
                                                    orb.bin_edges().ctypes.data_as(oracle.ctypes.c_void_p))


def oracle_harris(img, x, y, k):
    a = np.ascontiguousarray(img)
    return oracle.lib().kcmc_oracle_harris(a.ctypes.data_as(oracle.ctypes.c_void_p), a.shape[1], int(x), int(y), float(k))


def oracle_candidates(img, threshold=20, k=0.04, edge=16):
    """Every candidate (unlimited budget) in candidate order with its Harris response."""
    kp, _ = oracle.orb_detect(img, n_features=UNLIMITED, threshold=threshold, harris_k=k, edge=edge,
                              pattern=orb.rotated_patterns(), bin_cs=orb.bin_edges())
    kp = kp.astype(np.int64)
    return kp, np.array([oracle_harris(img, x, y, k) for x, y in kp])


# ------------------------------------------------------------------ the restatement, memoised
# The FAST score map, the candidates and a keypoint's descriptor do not depend on the
# budget (the first two not on each other's parameters either), so the cases that share an
# image share them: the restatement runs once per image, not once per parameter set.
_RAW, _CANDS, _DES = {}, {}, {}


def _key(img):
    return (img.shape, img.tobytes())


def _raw(img):
    k = _key(img)
    if k not in _RAW:
        _RAW[k] = score_map_py(img)
    return _RAW[k]


def _describe(img, x, y):
    k = (_key(img), x, y)
    if k not in _DES:
        _DES[k] = describe_py(img, x, y)
    return _DES[k]


def restate(img, p, des_stride=1):
    """detect_py with the memoised parts: keypoints of every kept candidate, and the
    descriptors of every des_stride-th one (rows, des)."""
    k = (_key(img), p.fast_threshold, p.harris_k, p.edge)
    if k not in _CANDS:
        _CANDS[k] = candidates_py(img, _raw(img), p.fast_threshold, p.harris_k, p.edge)
    kept = select_py(_CANDS[k], p.n_features)
    rows = list(range(0, len(kept), des_stride))
    kp = np.array([(x, y) for _, x, y in kept], np.float64).reshape(-1, 2)
    des = np.array([_describe(img, kept[i][1], kept[i][2]) for i in rows], np.uint8).reshape(-1, 32)
    return kp, rows, des


# geometry cases that the (slow) restatement covers: the smallest frames, every W % 4, one and
# two tile columns, nty odd and even; the rest of the geometry is pinned GPU vs oracle only
RESTATED_GEOMETRY = {"geometry/49x33", "geometry/49x34", "geometry/49x35", "geometry/49x36", "geometry/49x65",
                     "geometry/33x67", "geometry/34x128"}
# descriptors of every 8th keypoint only (all keypoints still compared): thousands of keypoints
SPARSE_DESCRIPTORS = {f"ties/n={n}" for n in (TIES_CUTS[1], TIES_TOTAL - 1, TIES_TOTAL, TIES_TOTAL + 1)} | \
                     {f"dense/t={t}" for t in DENSE_THRESHOLDS}
RESTATED = [n for n in CASE_NAMES if not n.startswith("geometry/") or n in RESTATED_GEOMETRY]


@pytest.mark.parametrize("name", RESTATED)
def test_oracle_matches_restatement(name):
    _, imgs, p = case(name)
    for f in range(len(imgs)):
        kp, des = detect_oracle(imgs[f], p)
        kp2, rows, des2 = restate(imgs[f], p, 8 if name in SPARSE_DESCRIPTORS else 1)
        assert np.array_equal(kp, kp2), (name, f)
        assert np.array_equal(des[rows], des2), (name, f)
        assert (len(kp) == 0) == (name in EMPTY_CASES), (name, f, len(kp))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_is_not_vacuous(name):
    _, imgs, p = case(name)
    assert imgs.dtype == np.uint8 and imgs.ndim == 3 and imgs.flags.c_contiguous
    for f in range(len(imgs)):
        n = len(detect_oracle(imgs[f], p)[0])
        assert (n == 0) == (name in EMPTY_CASES), (name, f, n)


# ------------------------------------------------------------------ each case hits its edge
def test_single_pixel():
    img = single_pixel_img()
    kp, des = detect_oracle(img, _P())
    assert kp.tolist() == [[16.0, 16.0]]  # x = edge = W - edge - 1: the only admissible pixel
    assert moments_py(img, 16, 16) == (0, 0) and oracle_bin(img, 16, 16) == 0 and bin_py(0, 0) == 0
    assert fast_score_py(img, 16, 16) == 255
    for name in ("single_pixel/32x100", "single_pixel/100x32", "single_pixel/32x32"):
        _, imgs, p = case(name)
        assert imgs[0, 16, 16] == 255 and min(imgs.shape[1:]) == 2 * p.edge  # one short of the smallest frame
        assert len(detect_oracle(imgs[0], p)[0]) == 0


def test_compass_moments_lie_on_bin_edges():
    img = compass_img()
    kp, _ = detect_oracle(img, _P())
    kept = {(int(x), int(y)) for x, y in kp}
    cs = orb.bin_edges()
    for i, ((x, y), (dx, dy)) in enumerate(zip(COMPASS_DOTS, COMPASS_OFFSETS)):
        assert (x, y) in kept
        m10, m01 = moments_py(img, x, y)
        assert (m10, m01) == (90 * dx, 90 * dy)
        assert m10 == 0 or m01 == 0 or abs(m10) == abs(m01)
        # the moment vector is parallel to edge 4 i: the cross product the kernel tests is
        # zero up to the rounding of the edge's cos / sin, so either side of floor() is in play
        assert abs(m01 * cs[4 * i, 0] - m10 * cs[4 * i, 1]) <= 1e-12 * 90 * 7 * 2
        assert oracle_bin(img, x, y) == 4 * i == bin_py(m10, m01)


def test_seams_ties_resolve_to_the_first_in_raster_order():
    img = seams_img()
    kp, _ = detect_oracle(img, _P())
    assert sorted((int(y), int(x)) for x, y in kp) == sorted((y, x) for y, x, _ in SEAM_SQUARES)
    for y, x, n in SEAM_SQUARES:
        s = [fast_score_py(img, x + dx, y + dy) for dy in range(n) for dx in range(n)]
        assert s == [200] * (n * n)  # a real tie: every pixel of the square scores the same
        tiles = {((y + dy) // 16, (x + dx) // 64) for dy in range(n) for dx in range(n)}
        regions = {(y + dy) // 32 for dy in range(n)}
        assert len(tiles) > 1 or len(regions) > 1
    y, x, n = SEAM_SQUARES[0]  # the winner's tied neighbours: the next tile column and the next region
    assert (x // 64, (x + 1) // 64) == (0, 1) and (y // 32, (y + 1) // 32) == (0, 1) and n == 2


def test_geometry_covers_every_path():
    shapes = set(GEOMETRY_SHAPES)
    assert len(shapes) == len(GEOMETRY_SHAPES) == 24
    nty = {-(-H // 16) for H, _ in shapes}
    assert {n % 2 for n in nty} == {0, 1}                            # the last region holds one tile, or two
    assert {W % 4 for _, W in shapes} == {0, 1, 2, 3}               # word and byte staging
    assert {-(-W // 64) for _, W in shapes} == {1, 2, 3}             # tile columns
    assert {(33, 67), (49, 33)} <= shapes                            # the smallest admissible H and W
    for H, W in shapes:
        a = geometry_imgs(H, W)
        assert not np.array_equal(a[0], a[1])


def test_edges_counts():
    img = edges_img()
    n = [len(detect_oracle(img, _P(edge=e))[0]) for e in EDGES]
    assert n[:3] == [500, 500, 500] and 0 < n[4] < n[3] < 500 and n[5] == 0, n
    assert img.shape[0] == 2 * 60 and img.shape[0] == 2 * 59 + 2   # edge 60: too small; 59: two admissible rows


def test_threshold_cases():
    img = binary_blocks_img()
    assert set(np.unique(img)) == {0, 255}
    kp, _ = oracle_candidates(img, threshold=0)
    assert len(kp) > 100
    assert {fast_score_py(img, x, y) for x, y in kp} == {255}  # every corner scores 255: kept up to 254, not at 255
    for t in THRESHOLDS:
        n = len(detect_oracle(img, _P(fast_threshold=t))[0])
        assert n == (0 if t == 255 else len(kp)), (t, n)


def test_harris_sign_cases():
    img = binary_blocks_img()
    kp, _ = oracle_candidates(img)
    r = {k: np.array([harris_py(img, x, y, k) for x, y in kp]) for k in HARRIS_KS + (HARRIS_K_MIXED,)}
    assert (r[0.0] > 0).all() and (r[0.04] > 0).all() and (r[0.25] < 0).all()
    m = r[HARRIS_K_MIXED]
    assert (m > 0).sum() == HARRIS_N_POS and (m < 0).sum() == len(kp) - HARRIS_N_POS > 0 and HARRIS_N_POS > 1
    # the budgets around the sign change keep exactly the positives, one fewer, one negative more
    for d in (-1, 0, 1):
        k2, _ = detect_oracle(img, _P(harris_k=HARRIS_K_MIXED, n_features=HARRIS_N_POS + d))
        rk = np.array([harris_py(img, int(x), int(y), HARRIS_K_MIXED) for x, y in k2])
        assert len(k2) == HARRIS_N_POS + d and (rk < 0).sum() == max(d, 0)


def test_ties_cases():
    img = ties_img()
    kp, r = oracle_candidates(img)
    vals, cnt = np.unique(r, return_counts=True)
    assert len(kp) == TIES_TOTAL and len(vals) <= 9 and cnt.max() >= 257, (len(kp), vals, cnt)
    for n in TIES_CUTS:
        T = np.sort(r)[::-1][n - 1]
        group, n_gt = int((r == T).sum()), int((r > T).sum())
        taken = n - n_gt
        assert group == cnt.max() and 256 < taken < group, (n, group, taken)
        # the ties taken are the first ones in candidate order, and they span several 256-candidate chunks
        k2, _ = detect_oracle(img, _P(n_features=n))
        want = np.concatenate([np.flatnonzero(r > T), np.flatnonzero(r == T)[:taken]])
        want.sort()
        assert np.array_equal(k2, kp[want].astype(np.float64))
        tie_rows = np.flatnonzero(r == T)[:taken]
        assert len(set(tie_rows // 256)) > 1
    assert TIES_CUTS[0] < cnt.max() < TIES_CUTS[1]  # the cut in the best group (nothing above T), and below it


def test_dense_tile_holds_over_100_candidates():
    img = dense_img()
    H, W = img.shape
    for t in DENSE_THRESHOLDS:
        kp, _ = oracle_candidates(img, threshold=t)
        tile = (kp[:, 1] // 16) * -(-W // 64) + kp[:, 0] // 64
        assert 100 <= np.bincount(tile).max() <= 256, (t, np.bincount(tile).max())


def test_every_orientation_bin_occurs():
    seen = set()
    for _, imgs, p in cases():
        for img in imgs:
            kp, _ = detect_oracle(img, p)
            seen |= {oracle_bin(img, x, y) for x, y in kp[:600]}
    assert seen == set(range(32))
