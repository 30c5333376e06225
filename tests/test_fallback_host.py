"""The intensity fallback (kcmc_amd.fallback, csrc/shift_search.hip) restated in numpy /
Python integers, and the host half of the module checked against the restatement (no GPU).

Build-defined semantics (the reference has no such mode), pinned here:
  search   out[k][dy + R][dx + R] = (Sa, Sb, Saa, Sbb, Sab) over the rectangle with
           a = frame[idx[k]][y + dy][x + dx], b = ref[y][x]; an index outside the stack is a
           zero row
  pick     the largest r (NaN = -inf), ties to the smaller dy^2 + dx^2, then dy, then dx;
           rejected when NaN, <= min_corr or on the window's border; parabolic sub-pixel step
           per axis, clamped to +-0.5, 0 unless den < 0 and both neighbours are numbers
  compose  M' = M with the translation lowered by (dx, dy)
The restatement shares no code with kcmc_amd.fallback; tests/test_gpu_fallback.py imports it.
"""
import ctypes
import math
import os

import numpy as np
import pytest

import test_quality_host as qhost
from kcmc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def ref_shift_search(frames, idx, ref, region, R):
    """[len(idx), S, S, 5] Python ints (object array).  The int64 partial sums are exact:
    a rectangle of n < 2^31 pixels of products < 2^32 stays below 2^63."""
    frames, ref = np.asarray(frames), np.asarray(ref)
    y0, y1, x0, x1 = region
    S = 2 * R + 1
    b = ref[y0:y1, x0:x1].astype(np.int64)
    sb, sbb = int(b.sum()), int((b * b).sum())
    out = np.empty((len(idx), S, S, 5), object)
    out[...] = 0
    for k, f in enumerate(idx):
        if not 0 <= f < len(frames):
            continue
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                a = frames[f][y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int64)
                out[k, dy + R, dx + R] = [int(a.sum()), sb, int((a * a).sum()), sbb, int((a * b).sum())]
    return out


def ref_correlations(stats, n):
    """[k, S, S] float64 from the moments [k, S, S, 5] over n pixels."""
    k, S = stats.shape[:2]
    return qhost.ref_pearson(stats.reshape(-1, 5), n).reshape(k, S, S)


def ref_pick_shift(r, R, min_corr=0.0, subpixel=True):
    """(dx, dy, r_peak, accepted); dx = dy = NaN when rejected."""
    r = np.asarray(r, np.float64)
    cand = []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            v = r[dy + R, dx + R]
            cand.append((0 if np.isnan(v) else 1, -np.inf if np.isnan(v) else v, -(dy * dy + dx * dx), -dy, -dx))
    _, _, _, ndy, ndx = max(cand)
    dy, dx = -ndy, -ndx
    r0 = r[dy + R, dx + R]
    if np.isnan(r0) or r0 <= min_corr or abs(dy) == R or abs(dx) == R:
        return math.nan, math.nan, float(r0), False

    def delta(lo, hi):
        if np.isnan(lo) or np.isnan(hi):
            return 0.0
        den = lo - 2.0 * r0 + hi
        if den >= 0:
            return 0.0
        return float(np.clip(0.5 * (lo - hi) / den, -0.5, 0.5))

    sx = delta(r[dy + R, dx + R - 1], r[dy + R, dx + R + 1]) if subpixel else 0.0
    sy = delta(r[dy + R - 1, dx + R], r[dy + R + 1, dx + R]) if subpixel else 0.0
    return dx + sx, dy + sy, float(r0), True


def ref_compose(M, dx, dy):
    out = np.array(M, np.float64)
    out[0, 2] = out[0, 2] - dx
    out[1, 2] = out[1, 2] - dy
    return out


def ref_search_region(region, R):
    y0, y1, x0, x1 = region
    rect = (y0 + R, y1 - R, x0 + R, x1 - R)
    return rect if rect[1] - rect[0] >= 2 * R + 1 and rect[3] - rect[2] >= 2 * R + 1 else None


def ref_fallback_pass(aligned, sources, affines, skipped, warp, R, min_corr=0.0, subpixel=True, rate=1):
    """The whole pass from what a run WITHOUT the fallback returns (aligned frames, maps,
    skipped) and the source frames; ``warp(frame, M)`` is the frame warp.  Returns (aligned',
    affines', shifts [k, 2], correlations [k, 2], idxs)."""
    aligned = np.array(aligned, copy=True)
    affines = np.array(affines, np.float64, copy=True)
    n, H, W = aligned.shape
    skipped = [int(i) for i in skipped]
    shifts = np.full((len(skipped), 2), np.nan)
    corr = np.full((len(skipped), 2), np.nan)
    sel = np.zeros(n, bool)
    sel[qhost.ref_sel0(n, rate, skipped)] = True
    rect = ref_search_region(qhost.ref_valid_region(affines[:n], H, W), R)
    if not skipped or rect is None:
        return aligned, affines, shifts, corr, []
    mean0 = qhost.ref_mean_image(aligned, sel)
    stats = ref_shift_search(aligned, skipped, mean0, rect, R)
    r = ref_correlations(stats, (rect[1] - rect[0]) * (rect[3] - rect[2]))
    idxs = []
    for j, i in enumerate(skipped):
        dx, dy, r_peak, ok = ref_pick_shift(r[j], R, min_corr, subpixel)
        corr[j] = (r[j, R, R], r_peak)
        if ok:
            shifts[j] = (dx, dy)
            affines[i] = ref_compose(affines[i], dx, dy)
            aligned[i] = warp(np.asarray(sources[i]), affines[i])
            idxs.append(i)
    return aligned, affines, shifts, corr, idxs


def blocked_scene(shape, seed, sigma=0.0):
    """4 x 4-blocked uniform noise (the texture of test_gpu_quality._scene), float64, with
    optional Gaussian pixel noise; not clipped."""
    rng = np.random.default_rng(seed)
    H, W = shape
    lo = rng.integers(0, 60000, ((H + 3) // 4, (W + 3) // 4)).astype(np.float64)
    img = np.kron(lo, np.ones((4, 4)))[:H, :W]
    return img + rng.normal(0, sigma, (H, W)) if sigma else img


def to_u16(x):
    return np.clip(x, 0, 65535).astype(np.uint16)


# ------------------------------------------------------------------------- the tests
def test_fallback_module_is_exported():
    import kcmc_amd
    from kcmc_amd import fallback

    assert kcmc_amd.fallback is fallback
    for name in ("shift_search", "pick_shift", "compose", "correct_skipped"):
        assert callable(getattr(fallback, name)), name
    va = kcmc_amd.VideoAligner
    assert va.FALLBACK == "interpolate" and va.FALLBACK_RADIUS == 8
    assert va.FALLBACK_MIN_CORRELATION == 0.0 and va.FALLBACK_SUBPIXEL is True
    inst = va()
    for attr in ("fallback_shifts", "fallback_correlations", "fallback_idxs"):
        assert getattr(inst, attr) is None, attr


def test_header_and_binding_table_name_the_entry_point():
    with open(os.path.join(REPO, "include", "kcmc.h")) as fh:
        header = fh.read()
    assert "int kcmc_shift_search_u16(kcmc_ctx* ctx, const uint16_t* frames_dev, int n_frames, int H, int W," in header
    assert "#define KCMC_ABI_VERSION 2" in header
    assert "kcmc_shift_search_u16" in _lib.EXPORTED_SYMBOLS and "kcmc_shift_search_u16" in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["kcmc_shift_search_u16"][0]) == 15
    assert _lib.ABI_VERSION == 2
    L = _lib.load()
    assert L.kcmc_abi_version() == 2 and hasattr(L, "kcmc_shift_search_u16")


def _pick(r, R, min_corr=0.0, subpixel=True):
    from kcmc_amd import fallback

    got = fallback.pick_shift(np.asarray(r, np.float64), R, min_corr, subpixel)
    want = ref_pick_shift(r, R, min_corr, subpixel)
    np.testing.assert_array_equal(np.array(got[:3]), np.array(want[:3]))  # NaN == NaN here
    assert got.accepted == want[3]
    return got


def test_pick_shift_tie_break_order():
    R = 2
    r = np.full((5, 5), 0.1)
    # four equal peaks at distance^2 = 2 and one at distance^2 = 1: the nearest wins
    for dy, dx in ((-1, -1), (-1, 1), (1, -1), (1, 1), (0, 1)):
        r[dy + R, dx + R] = 0.9
    p = _pick(r, R, subpixel=False)
    assert (p.dx, p.dy, p.accepted) == (1.0, 0.0, True)
    r[0 + R, 1 + R] = 0.1  # equal distance: the smaller dy, then the smaller dx
    p = _pick(r, R, subpixel=False)
    assert (p.dx, p.dy) == (-1.0, -1.0)
    r[-1 + R, -1 + R] = 0.1
    p = _pick(r, R, subpixel=False)
    assert (p.dx, p.dy) == (1.0, -1.0)
    r[-1 + R, 1 + R] = 0.1
    p = _pick(r, R, subpixel=False)
    assert (p.dx, p.dy) == (-1.0, 1.0)
    # a flat window: the zero shift
    p = _pick(np.full((5, 5), 0.5), R)
    assert (p.dx, p.dy, p.r_peak, p.accepted) == (0.0, 0.0, 0.5, True)


def test_pick_shift_nan_border_and_min_corr():
    R = 3
    S = 2 * R + 1
    p = _pick(np.full((S, S), np.nan), R)
    assert not p.accepted and math.isnan(p.dx) and math.isnan(p.dy) and math.isnan(p.r_peak)
    r = np.full((S, S), np.nan)
    r[1 + R, -2 + R] = -0.5  # the only number is the peak: NaN counts as -inf
    p = _pick(r, R, min_corr=-1.0)
    assert (p.dx, p.dy, p.r_peak, p.accepted) == (-2.0, 1.0, -0.5, True)  # NaN neighbours: no sub-pixel step
    assert not _pick(r, R, min_corr=0.0).accepted
    assert not _pick(r, R, min_corr=-0.5).accepted  # r <= min_corr rejects
    for dy, dx in ((-R, 0), (R, 1), (0, -R), (2, R), (R, R)):  # the border: a saturated search
        r = np.full((S, S), 0.2)
        r[dy + R, dx + R] = 0.9
        p = _pick(r, R)
        assert not p.accepted and p.r_peak == 0.9 and math.isnan(p.dx)
    r = np.full((S, S), 0.2)
    r[(R - 1) + R, -(R - 1) + R] = 0.9  # one inside the border is fine
    p = _pick(r, R, subpixel=False)
    assert (p.dx, p.dy, p.accepted) == (-(R - 1.0), R - 1.0, True)


def test_pick_shift_subpixel():
    R = 2
    r = np.zeros((5, 5))
    r[R, R], r[R, R - 1], r[R, R + 1], r[R - 1, R], r[R + 1, R] = 1.0, 0.5, 0.75, 0.25, 0.25
    p = _pick(r, R)
    # x: den = 0.5 - 2 + 0.75 = -0.75, delta = 0.5 * (0.5 - 0.75) / -0.75 = 1/6; y: symmetric, 0
    assert p.dx == pytest.approx(1 / 6, abs=1e-15) and p.dy == 0.0
    assert _pick(r, R, subpixel=False).dx == 0.0
    # den >= 0 (a tie with a neighbour on a plateau, chosen by the tie-break): no step
    r = np.zeros((5, 5))
    r[R, R] = r[R, R + 1] = r[R, R - 1] = 0.8
    p = _pick(r, R)
    assert (p.dx, p.dy) == (0.0, 0.0)
    # the ends of the clamp: no neighbour exceeds the peak, so the vertex reaches +-0.5 only when
    # a neighbour ties with it (the tie-break picked the nearer one): (0.25, 0.75, 0.75) -> +0.5
    r = np.full((5, 5), 0.0)
    r[R, R], r[R, R + 1], r[R, R - 1] = 0.75, 0.75, 0.25
    assert _pick(r, R).dx == 0.5
    r = np.full((5, 5), -1.0)
    r[R, R], r[R - 1, R], r[R + 1, R] = 0.5, 0.5 - 1e-9, -1.0  # den = -1.5 - 1e-9: just inside -0.5
    p = _pick(r, R)
    assert -0.5 <= p.dy < -0.49 and p.dx == 0.0
    rng = np.random.default_rng(4)
    for _ in range(300):  # random windows, some with NaN and ties
        R = int(rng.integers(1, 5))
        S = 2 * R + 1
        r = np.round(rng.uniform(-1, 1, (S, S)), 1)
        r[rng.random((S, S)) < 0.1] = np.nan
        p = _pick(r, R, min_corr=float(rng.choice([-2.0, 0.0, 0.5])), subpixel=bool(rng.integers(0, 2)))
        if p.accepted:
            assert abs(p.dx - round(p.dx)) <= 0.5 and abs(p.dy - round(p.dy)) <= 0.5


def test_pick_shift_rejects_bad_arguments():
    from kcmc_amd import fallback

    with pytest.raises(ValueError):
        fallback.pick_shift(np.zeros((5, 5)), 3)
    for radius in (0, 17, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            fallback.check_radius(radius)
    assert fallback.check_radius(1) == 1 and fallback.check_radius(np.int64(16)) == 16
    assert fallback.search_region((7, 89, 7, 153), 8) == (15, 81, 15, 145) == ref_search_region((7, 89, 7, 153), 8)
    assert fallback.search_region((0, 33, 0, 40), 8) == (8, 25, 8, 32)  # 17 rows: just enough
    assert fallback.search_region((0, 32, 0, 40), 8) is None and ref_search_region((0, 32, 0, 40), 8) is None
    assert fallback.search_region((0, 40, 0, 32), 8) is None


def test_compose_signs_against_the_matrix_identity():
    """M' = T(-d) M as 3 x 3 matrices: the corrected frame is src(M^-1(p + d)), so
    M'^-1 = M^-1 T(d)."""
    from kcmc_amd import fallback

    rng = np.random.default_rng(2)
    for _ in range(20):
        th = rng.uniform(-0.2, 0.2)
        c, s = math.cos(th), math.sin(th)
        M = np.array([[c, -s, rng.uniform(-9, 9)], [s, c, rng.uniform(-9, 9)]])
        dx, dy = rng.uniform(-8, 8, 2)
        got = fallback.compose(M, dx, dy)
        np.testing.assert_array_equal(got, ref_compose(M, dx, dy))
        assert got.dtype == np.float64 and got is not M
        M3, T = np.vstack([M, [0, 0, 1]]), np.array([[1, 0, -dx], [0, 1, -dy], [0, 0, 1]])
        np.testing.assert_allclose(np.vstack([got, [0, 0, 1]]), T @ M3, rtol=0, atol=1e-15)
        p = rng.uniform(0, 100, 2)
        src_of = lambda A, q: np.linalg.solve(np.vstack([A, [0, 0, 1]]), [q[0], q[1], 1.0])[:2]  # noqa: E731
        np.testing.assert_allclose(src_of(got, p), src_of(M, p + [dx, dy]), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        fallback.compose(np.eye(3), 1, 1)


# The scene of the issue: 4 x 4-blocked noise, a 96 x 160 crop, R = 8; the reference is the
# clean crop, the frame the crop displaced by an offset with pixel noise of sigma on top.
H, W, R, PAD = 96, 160, 8, 16
RECT = (R + 1, H - R - 1, R + 1, W - R - 1)
N = (RECT[1] - RECT[0]) * (RECT[3] - RECT[2])


def _search_one(sigma, off, divide=1, seed=7):
    """off = (dx, dy): the frame's content is the reference's displaced by -off, so that
    frame(p + off) = ref(p)."""
    clean = blocked_scene((H + 2 * PAD, W + 2 * PAD), seed)
    ref = to_u16(clean[PAD:PAD + H, PAD:PAD + W])
    dx, dy = off
    rng = np.random.default_rng(seed + 1)
    frame = to_u16(clean[PAD - dy:PAD - dy + H, PAD - dx:PAD - dx + W] + rng.normal(0, sigma, (H, W))) // divide
    stats = ref_shift_search(frame[None], [0], ref, RECT, R)
    return ref_correlations(stats, N)[0]


@pytest.mark.parametrize("sigma", [800, 8000, 30000])
def test_restated_search_finds_the_offset_under_noise(sigma):
    from kcmc_amd import fallback

    for off in ((0, 0), (3, -5), (-7, 7), (7, -1)):
        r = _search_one(sigma, off)
        got = fallback.pick_shift(r, R, 0.0, subpixel=False)
        runner_up = np.sort(r.ravel())[-2]
        print("sigma", sigma, "offset", off, "peak r", got.r_peak, "runner-up", runner_up)
        assert got.accepted and (got.dx, got.dy) == off
        assert got.r_peak == r[off[1] + R, off[0] + R] > runner_up
        sub = _pick(r, R)  # with the parabola: within half a pixel of the truth
        assert abs(sub.dx - off[0]) <= 0.5 and abs(sub.dy - off[1]) <= 0.5


def test_restated_search_ignores_the_gain_and_rejects_the_border():
    from kcmc_amd import fallback

    r = _search_one(800, (-4, 6), divide=64)  # a dim frame: Pearson's r ignores the gain
    got = fallback.pick_shift(r, R, 0.0, subpixel=False)
    print("dim frame: peak r", got.r_peak)
    assert got.accepted and (got.dx, got.dy) == (-4, 6) and got.r_peak > 0.99
    for off in ((R, 0), (-2, -R), (R, R)):  # an offset of exactly R peaks on the border
        r = _search_one(800, off)
        got = _pick(r, R)
        assert not got.accepted and math.isnan(got.dx) and got.r_peak == r[off[1] + R, off[0] + R]


def test_entry_point_validates_before_touching_the_gpu():
    check_validation(ctypes.c_void_p(np.zeros(8, np.int64).ctypes.data), None)


def check_validation(ctx, good):
    """Every contract violation is KCMC_EINVAL before any device work.  ``ctx``: a context
    handle (never dereferenced by the checks); ``good``: device pointers (frames, idx, ref,
    out) of a valid 33 x 40 call, or None on a box without a GPU (a host buffer stands in:
    nothing reads it)."""
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(64, np.int64)
    fr, idx, ref, out = good if good is not None else (buf.ctypes.data,) * 4
    H, W = 33, 40

    def call(ctx=ctx, fr=fr, n_frames=1, H=H, W=W, idx=idx, n_sel=1, ref=ref, rect=(8, 25, 8, 32), R=8, out=out):
        p = lambda v: None if v is None else P(v)  # noqa: E731
        return L.kcmc_shift_search_u16(ctx, p(fr), n_frames, H, W, p(idx), n_sel, p(ref), *rect, R, p(out), None)

    E = _lib.KCMC_EINVAL
    assert call(ctx=None) == E and b"ctx" in L.kcmc_last_error()
    assert call(fr=None) == E and b"NULL" in L.kcmc_last_error()
    assert call(ref=None) == E
    assert call(out=None) == E
    assert call(out=out + 4) == E and b"aligned" in L.kcmc_last_error()
    for R in (0, 17, -3):
        assert call(R=R, rect=(17, 18, 17, 18), H=64, W=64) == E and b"R must" in L.kcmc_last_error()
    assert call(rect=(8, 8, 8, 32)) == E and b"empty" in L.kcmc_last_error()
    assert call(rect=(8, 25, 20, 19)) == E
    for rect in ((7, 25, 8, 32), (8, 26, 8, 32), (8, 25, 7, 32), (8, 25, 8, 33)):  # the halo leaves the image
        assert call(rect=rect) == E and b"leaves the image" in L.kcmc_last_error(), rect
    assert call(H=1 << 16, W=1 << 15) == E and b"2^31" in L.kcmc_last_error()
    assert call(n_sel=-1) == E and call(n_frames=-1) == E and call(H=0) == E
    assert call(n_sel=0) == _lib.KCMC_OK
    assert call(n_sel=0, fr=None, idx=None, ref=None, out=None) == _lib.KCMC_OK
    if good is not None:
        assert call() == _lib.KCMC_OK


def test_switch_checks_fail_before_any_work():
    from kcmc_amd import VideoAligner

    def va(**kw):
        return type("VA", (VideoAligner,), {"FALLBACK": "correlation", **kw})()

    stack4 = np.zeros((2, 4, 4, 3), np.uint16)
    for make, err, images in ((lambda: va(RANSAC_MODEL="projective"), NotImplementedError, None),
                              (lambda: va(PIECEWISE_GRID=(2, 2)), NotImplementedError, None),
                              (lambda: va(), NotImplementedError, stack4),
                              (lambda: va(FALLBACK_RADIUS=0), ValueError, None),
                              (lambda: va(FALLBACK_RADIUS=17), ValueError, None),
                              (lambda: va(FALLBACK="fft"), ValueError, None)):
        with pytest.raises(err, match="FALLBACK|fallback"):
            make().align_images(images, 10, "orb", 30)
        with pytest.raises(err, match="FALLBACK|fallback"):
            make().align_keypoints(images, None, None, None, None, 10)
