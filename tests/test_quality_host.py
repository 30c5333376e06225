"""The registration quality metrics restated in numpy / Python integers, and the host half
of kcmc_amd.quality checked against the restatement (no GPU).

The restatement below is the yardstick of tests/test_gpu_quality.py: integer sums (int64
where the bound F * 65535^2 * H * W < 2^63 makes it exact, Python ints from there on), the
rounded mean, the valid region, Pearson's r and the selection rule of the template
refinement.  It shares no code with kcmc_amd.quality.
"""
import ctypes
import math

import numpy as np
import pytest

from kcmc_amd import _lib


# ------------------------------------------------------------------ the restatement
def ref_stack_sum(frames, sel=None):
    """[H, W] int64: the sum over the selected frames (exact: F * 65535 < 2^63)."""
    frames = np.asarray(frames)
    sel = np.ones(len(frames), bool) if sel is None else np.asarray(sel, bool)
    return frames[sel].astype(np.int64).sum(axis=0).reshape(frames.shape[1:])


def ref_mean_image(frames, sel=None):
    n = len(frames) if sel is None else int(np.sum(sel))
    if n == 0:
        raise ValueError("no frame selected")
    return ((ref_stack_sum(frames, sel) + n // 2) // n).astype(np.uint16)


def ref_invert(M):
    """OpenCV warpAffine's inversion of a forward 2x3 map (float64, its order of operations)."""
    M = np.array(M, np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[1, 1] * D, M[0, 0] * D
    M[0, 0] = A11
    M[0, 1] *= -D
    M[1, 0] *= -D
    M[1, 1] = A22
    b1 = -M[0, 0] * M[0, 2] - M[0, 1] * M[1, 2]
    b2 = -M[1, 0] * M[0, 2] - M[1, 1] * M[1, 2]
    M[0, 2], M[1, 2] = b1, b2
    return M


def ref_valid_region(affines, H, W):
    """m = ceil(d) + 1 with d the largest corner displacement, where a d that float64
    evaluates up to (H + W) * 2^-40 px above an integer counts as that integer (rounding
    dust of an estimated map; the margin argument needs only m > d + 1/16)."""
    affines = np.asarray(affines, np.float64)
    if affines.shape[1:] == (3, 3):
        raise NotImplementedError
    if not np.isfinite(affines).all():
        raise ValueError("non-finite affine")
    d = 0.0
    for M in affines:
        inv = ref_invert(M)
        for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            sx = inv[0, 0] * cx + inv[0, 1] * cy + inv[0, 2]
            sy = inv[1, 0] * cx + inv[1, 1] * cy + inv[1, 2]
            d = max(d, abs(sx - cx), abs(sy - cy))
    m = math.ceil(d - (H + W) * 2.0 ** -40) + 1
    if 2 * m >= min(H, W):
        raise ValueError("no common valid region")
    return m, H - m, m, W - m


def ref_frame_stats(frames, ref, region):
    """[F, 5] Python ints (object array): (Sa, Sb, Saa, Sbb, Sab) over the region."""
    y0, y1, x0, x1 = region
    b = np.asarray(ref)[y0:y1, x0:x1].astype(np.int64)
    out = np.empty((len(frames), 5), object)
    for f, fr in enumerate(np.asarray(frames)):
        a = fr[y0:y1, x0:x1].astype(np.int64)
        out[f] = [int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum())]
    return out


def ref_pearson(stats, n):
    out = np.full(len(stats), np.nan)
    for f, (sa, sb, saa, sbb, sab) in enumerate(stats):
        sa, sb, saa, sbb, sab = int(sa), int(sb), int(saa), int(sbb), int(sab)
        num = n * sab - sa * sb
        va = n * saa - sa * sa
        vb = n * sbb - sb * sb
        if va != 0 and vb != 0:
            out[f] = float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb)))
    return out


def ref_correlations(frames, ref, region):
    y0, y1, x0, x1 = region
    return ref_pearson(ref_frame_stats(frames, ref, region), (y1 - y0) * (x1 - x0))


def ref_sel0(n_images, rate, skipped):
    return [i for i in range(n_images) if i % rate == 0 and i not in set(skipped)]


def ref_select_top(corr, sel0, top_frac):
    order = sorted(sel0, key=lambda i: (-(-math.inf if math.isnan(corr[i]) else corr[i]), i))
    return order[:max(1, math.ceil(top_frac * len(sel0)))]


def ref_pass_metrics(aligned, affines, skipped, rate=1):
    """(mean image, region, correlations, sel0) of one pass, from what it returns."""
    aligned = np.asarray(aligned)
    n, H, W = aligned.shape
    sel0 = ref_sel0(n, rate, skipped)
    sel = np.zeros(n, bool)
    sel[sel0] = True
    mean0 = ref_mean_image(aligned, sel)
    region = ref_valid_region(np.asarray(affines)[:n], H, W)
    return mean0, region, ref_correlations(aligned, mean0, region), sel0


def ref_refined_template(aligned, corr, sel0, top_frac=0.5):
    best = np.zeros(len(aligned), bool)
    best[ref_select_top(corr, sel0, top_frac)] = True
    return ref_mean_image(aligned, best)


# ------------------------------------------------------------------------- the tests
def test_quality_module_is_exported():
    import kcmc_amd
    from kcmc_amd import quality

    assert kcmc_amd.quality is quality
    for name in ("stack_sum", "mean_image", "valid_region", "frame_stats", "pearson", "frame_correlations"):
        assert callable(getattr(quality, name)), name
    va = kcmc_amd.VideoAligner
    assert va.QUALITY_METRICS is False and va.TEMPLATE_REFINE_ITERS == 0 and va.TEMPLATE_REFINE_TOP_FRAC == 0.5
    inst = va()
    for attr in ("frame_correlations", "mean_image", "valid_region", "template_image", "correlation_history"):
        assert getattr(inst, attr) is None, attr


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pearson_matches_corrcoef(seed):
    from kcmc_amd import quality

    rng = np.random.default_rng(seed)
    F, H, W = 4, 37, 53
    ref = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    frames = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    frames[1] = np.clip(ref.astype(np.int64) + rng.integers(-2000, 2000, (H, W)), 0, 65535).astype(np.uint16)
    frames[2] = 65535 - ref  # r = -1
    region = (3, H - 2, 5, W - 4)
    stats = ref_frame_stats(frames, ref, region)
    n = (region[1] - region[0]) * (region[3] - region[2])
    r = quality.pearson(stats, n)
    np.testing.assert_array_equal(r, ref_pearson(stats, n))
    b = ref[region[0]:region[1], region[2]:region[3]].astype(np.float64).ravel()
    want = [np.corrcoef(fr[region[0]:region[1], region[2]:region[3]].astype(np.float64).ravel(), b)[0, 1]
            for fr in frames]
    np.testing.assert_allclose(r, want, rtol=1e-12, atol=0)
    assert r[2] == pytest.approx(-1.0, abs=1e-12)
    # int64 moments (what the kernel hands back) give the same numbers
    np.testing.assert_array_equal(quality.pearson(stats.astype(np.int64), n), r)


def test_pearson_constant_frame_is_nan_and_large_frames_do_not_overflow():
    from kcmc_amd import quality

    rng = np.random.default_rng(3)
    ref = rng.integers(0, 65536, (8, 8)).astype(np.uint16)
    frames = np.stack([np.full((8, 8), 1234, np.uint16), ref])
    r = quality.pearson(ref_frame_stats(frames, ref, (0, 8, 0, 8)), 64)
    assert math.isnan(r[0]) and r[1] == pytest.approx(1.0, abs=1e-15)
    assert math.isnan(quality.pearson(ref_frame_stats(frames[1:], frames[0], (0, 8, 0, 8)), 64)[0])  # constant ref
    # an all-65535 1080 x 1920 frame against an all-65535 reference, by the closed-form sums:
    # n * Sab = n^2 * 65535^2 ~ 2^74 must not wrap; both variances are exactly 0 -> NaN
    n, v = 1080 * 1920, 65535
    full = np.array([[n * v, n * v, n * v * v, n * v * v, n * v * v]], np.int64)
    assert math.isnan(quality.pearson(full, n)[0])
    # the same frame with one pixel at 0 in both: r is exactly 1, far from what wrapped sums give
    one = np.array([[(n - 1) * v, (n - 1) * v, (n - 1) * v * v, (n - 1) * v * v, (n - 1) * v * v]], np.int64)
    assert quality.pearson(one, n)[0] == pytest.approx(1.0, abs=1e-15)
    # ... and against a reference with that pixel at 65535 and another at 0: r = -1 / (n - 1)
    two = np.array([[(n - 1) * v, (n - 1) * v, (n - 1) * v * v, (n - 1) * v * v, (n - 2) * v * v]], np.int64)
    assert quality.pearson(two, n)[0] == pytest.approx(-1.0 / (n - 1), rel=1e-12)


def _rigid(theta, tx, ty):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]])


def test_valid_region_is_free_of_border_taps():
    from kcmc_amd import quality

    rng = np.random.default_rng(11)
    H, W = 60, 80
    for _ in range(2000):
        M = _rigid(rng.uniform(-0.05, 0.05), rng.uniform(-6, 6), rng.uniform(-6, 6))
        region = quality.valid_region(M[None], H, W)
        assert region == ref_valid_region(M[None], H, W)
        y0, y1, x0, x1 = region
        inv = ref_invert(M)
        ys, xs = np.mgrid[y0:y1, x0:x1]
        sx = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2]
        sy = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]
        # both bilinear taps inside the source, with the warp's 1/32 px fixed point as slack
        assert np.floor(sx - 1 / 32).min() >= 0 and np.floor(sx + 1 / 32).max() <= W - 2
        assert np.floor(sy - 1 / 32).min() >= 0 and np.floor(sy + 1 / 32).max() <= H - 2


def test_valid_region_edge_cases():
    from kcmc_amd import quality

    H, W = 60, 80
    ident = _rigid(0, 0, 0)
    assert quality.valid_region(ident[None], H, W) == (1, H - 1, 1, W - 1)
    assert quality.valid_region(np.zeros((0, 2, 3)), H, W) == (1, H - 1, 1, W - 1)
    # the largest displacement over the frames counts; integer shifts are exact
    maps = np.stack([ident, _rigid(0, 6, -2), _rigid(0, -3, 5)])
    assert quality.valid_region(maps, 200, 260) == (7, 193, 7, 253) == ref_valid_region(maps, 200, 260)
    assert quality.valid_region(_rigid(0, 6.25, 0)[None], H, W) == (8, H - 8, 8, W - 8)
    assert quality.valid_region(_rigid(0, 6 + 1e-6, 0)[None], H, W) == (8, H - 8, 8, W - 8)
    # an estimated map: an exact shift of (6, 5) beside a rotation of 3.5e-18 rad evaluates to a
    # displacement of 6.000000000000001 at the corner (0, 199); the last bit costs no margin
    dust = np.array([[1, 3.524210024144931e-18, 6], [-3.524210024144931e-18, 1, 5 - 3.552713678800501e-15]])
    inv = ref_invert(dust)
    assert abs(inv[0, 1] * 199 + inv[0, 2]) > 6
    assert quality.valid_region(dust[None], 200, 260) == (7, 193, 7, 253) == ref_valid_region(dust[None], 200, 260)
    with pytest.raises(ValueError, match="no common valid region"):
        quality.valid_region(_rigid(0, 40, 0)[None], H, W)
    with pytest.raises(ValueError, match="no common valid region"):
        quality.valid_region(_rigid(0, 0, 28.5)[None], H, W)  # m = 30: 2 m = H
    assert quality.valid_region(_rigid(0, 0, 28)[None], H, W) == (29, 31, 29, 51)
    bad = np.stack([ident, ident])
    bad[1, 0, 2] = np.nan
    with pytest.raises(ValueError):
        quality.valid_region(bad, H, W)
    bad[1, 0, 2] = np.inf
    with pytest.raises(ValueError):
        quality.valid_region(bad, H, W)
    with pytest.raises(NotImplementedError):
        quality.valid_region(np.eye(3)[None], H, W)


def test_selection_rule():
    from kcmc_amd import quality

    corr = np.array([0.5, 0.9, np.nan, 0.9, 0.7, 0.1])
    for sel0, frac, want in [
        ([0, 1, 2, 3, 4, 5], 0.5, [1, 3, 4]),       # ties to the lower index
        ([0, 1, 2, 3, 4, 5], 1.0, [1, 3, 4, 0, 5, 2]),  # NaN last
        ([0, 2, 5], 0.5, [0, 5]),                    # ceil(1.5) = 2
        ([2, 5], 0.5, [5]),                          # ceil(1.0) = 1
        ([2], 0.5, [2]),                             # max(1, ceil(0.5)) = 1, NaN or not
        ([3, 1], 0.5, [1]),
        ([0, 1, 3], 0.01, [1]),
    ]:
        assert quality.select_top(corr, sel0, frac) == want == ref_select_top(corr, sel0, frac), (sel0, frac)
    with pytest.raises(ValueError):
        quality.select_top(corr, [], 0.5)
    assert ref_sel0(7, 2, [2]) == [0, 4, 6] and ref_sel0(5, 1, []) == [0, 1, 2, 3, 4]


def test_restated_mean_rounds_half_up():
    frames = np.array([[[0, 1, 65535]], [[1, 2, 65535]], [[1, 1, 65534]]], np.uint16)
    np.testing.assert_array_equal(ref_mean_image(frames), [[1, 1, 65535]])            # 2/3, 4/3, 196604/3
    np.testing.assert_array_equal(ref_mean_image(frames[:2]), [[1, 2, 65535]])        # 1/2 and 3/2 round up
    np.testing.assert_array_equal(ref_mean_image(frames, [True, False, True]), [[1, 1, 65535]])
    with pytest.raises(ValueError):
        ref_mean_image(frames, [False, False, False])


def test_new_entry_points_validate_before_touching_the_gpu():
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(P)
    fake_ctx = P(buf.ctypes.data)  # never dereferenced: the argument checks come first
    assert L.kcmc_stack_sum_u16(None, p, 1, 8, None, p, None) == _lib.KCMC_EINVAL
    assert b"ctx" in L.kcmc_last_error()
    assert L.kcmc_stack_sum_u16(fake_ctx, None, 1, 8, None, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_stack_sum_u16(fake_ctx, p, 1, 8, None, None, None) == _lib.KCMC_EINVAL
    assert L.kcmc_stack_sum_u16(fake_ctx, p, 1, 0, None, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_stack_sum_u16(fake_ctx, p, -1, 8, None, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_frame_stats_u16(None, p, 1, 4, 4, p, 0, 4, 0, 4, p, None) == _lib.KCMC_EINVAL
    assert b"ctx" in L.kcmc_last_error()
    assert L.kcmc_frame_stats_u16(fake_ctx, None, 1, 4, 4, p, 0, 4, 0, 4, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 4, 4, p, 0, 4, 0, 4, None, None) == _lib.KCMC_EINVAL
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 4, 4, p, 2, 2, 0, 4, p, None) == _lib.KCMC_EINVAL  # empty
    assert b"empty" in L.kcmc_last_error()
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 4, 4, p, 0, 4, 3, 1, p, None) == _lib.KCMC_EINVAL
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 4, 4, p, 0, 5, 0, 4, p, None) == _lib.KCMC_EINVAL  # outside
    assert L.kcmc_frame_stats_u16(fake_ctx, p, 1, 1 << 16, 1 << 15, p, 0, 4, 0, 4, p, None) == _lib.KCMC_EINVAL
    assert b"2^31" in L.kcmc_last_error()


def test_switch_checks_fail_before_any_work():
    """projective + either switch, and refinement without a detector, raise from the public
    entry points before they look at their inputs (no GPU is touched)."""
    from kcmc_amd import VideoAligner

    class Proj(VideoAligner):
        RANSAC_MODEL = "projective"
        QUALITY_METRICS = True

    class ProjRefine(VideoAligner):
        RANSAC_MODEL = "projective"
        TEMPLATE_REFINE_ITERS = 1

    class Refine(VideoAligner):
        TEMPLATE_REFINE_ITERS = 1

    for cls in (Proj, ProjRefine):
        with pytest.raises(NotImplementedError):
            cls().align_images(None, 10, "orb", 30)
        with pytest.raises(NotImplementedError):
            cls().align_keypoints(None, None, None, None, None, 10)
    with pytest.raises(ValueError, match="TEMPLATE_REFINE_ITERS"):
        Refine().align_keypoints(None, None, None, None, None, 10)
