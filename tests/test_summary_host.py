"""The summary images restated in numpy / Python integers, and the host half of
kcmc_amd.summary checked against the restatement (no GPU).

The restatement below is the yardstick of tests/test_gpu_summary.py: the temporal planes and
the max of a stack as include/kcmc.h defines them (int64 sums of int64 products, exact while
F * 65535^2 < 2^63), and the four finishing functions pixel by pixel on Python ints.  It
shares no code with kcmc_amd.summary.
"""
import ctypes
import math

import numpy as np
import pytest

from kcmc_amd import _lib

# the partner of planes 2, 3, 4, 5 and, for the correlation image, the order of the neighbours
PARTNERS = ((0, 1), (1, 0), (1, 1), (1, -1))
NEIGHBOUR_ORDER = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))


# ------------------------------------------------------------------ the restatement
def ref_temporal_sums(frames, region, sel=None, neighbours=8):
    """(n, planes [K, H, W] int64, max [H, W] uint16) of the selected frames over the region."""
    frames = np.asarray(frames)
    F, H, W = frames.shape
    sel = np.ones(F, bool) if sel is None else np.asarray(sel, bool)
    y0, y1, x0, x1 = region
    a = np.zeros((int(sel.sum()), H, W), np.int64)
    a[:, y0:y1, x0:x1] = frames[sel][:, y0:y1, x0:x1]
    planes = np.zeros((2 + neighbours // 2, H, W), np.int64)
    planes[0] = a.sum(axis=0)
    planes[1] = (a * a).sum(axis=0)
    padded = np.pad(a, ((0, 0), (1, 1), (1, 1)))  # a is 0 outside the region, and so is every product with it
    for k, (dy, dx) in enumerate(PARTNERS[:neighbours // 2]):
        planes[2 + k] = (a * padded[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]).sum(axis=0)
    top = a.max(axis=0).astype(np.uint16) if len(a) else np.zeros((H, W), np.uint16)
    return len(a), planes, top


def ref_mean_image(planes, n, region):
    y0, y1, x0, x1 = region
    out = np.zeros(planes.shape[1:], np.uint16)
    for y in range(y0, y1):
        for x in range(x0, x1):
            out[y, x] = (int(planes[0, y, x]) + n // 2) // n
    return out


def ref_std_image(planes, n, region):
    y0, y1, x0, x1 = region
    out = np.full(planes.shape[1:], np.nan)
    for y in range(y0, y1):
        for x in range(x0, x1):
            s0, s1 = int(planes[0, y, x]), int(planes[1, y, x])
            out[y, x] = math.sqrt(float(n * s1 - s0 * s0)) / n
    return out


def _pair_sum(planes, y, x, dy, dx):
    """sum a(y, x) a(y + dy, x + dx): the plane of (dy, dx) at p, or of (-dy, -dx) at the partner."""
    if (dy, dx) in PARTNERS:
        return int(planes[2 + PARTNERS.index((dy, dx)), y, x])
    return int(planes[2 + PARTNERS.index((-dy, -dx)), y + dy, x + dx])


def ref_correlation_image(planes, n, region):
    y0, y1, x0, x1 = region
    nb = 2 * (planes.shape[0] - 2)
    out = np.full(planes.shape[1:], np.nan)
    var = [[n * int(planes[1, y, x]) - int(planes[0, y, x]) ** 2 for x in range(planes.shape[2])]
           for y in range(planes.shape[1])]
    for y in range(y0, y1):
        for x in range(x0, x1):
            total, count = 0.0, 0
            for dy, dx in NEIGHBOUR_ORDER[:nb]:
                qy, qx = y + dy, x + dx
                if not (y0 <= qy < y1 and x0 <= qx < x1):
                    continue
                vp, vq = var[y][x], var[qy][qx]
                if vp == 0 or vq == 0:
                    continue
                num = n * _pair_sum(planes, y, x, dy, dx) - int(planes[0, y, x]) * int(planes[0, qy, qx])
                total += float(num) / (math.sqrt(float(vp)) * math.sqrt(float(vq)))
                count += 1
            if count:
                out[y, x] = total / count
    return out


def ref_crispness(mean_u16, region):
    y0, y1, x0, x1 = region
    if y1 - y0 < 3 or x1 - x0 < 3:
        return math.nan
    total = 0
    for y in range(y0 + 1, y1 - 1):
        for x in range(x0 + 1, x1 - 1):
            gx = int(mean_u16[y, x + 1]) - int(mean_u16[y, x - 1])
            gy = int(mean_u16[y + 1, x]) - int(mean_u16[y - 1, x])
            total += gx * gx + gy * gy
    return math.sqrt(float(total)) / 2


def ref_summary(aligned, region, neighbours=8):
    """What VideoAligner leaves with SUMMARY_IMAGES on, from the aligned stack it returns."""
    n, planes, top = ref_temporal_sums(aligned, region, None, neighbours)
    mean = ref_mean_image(planes, n, region)
    return {"summary_mean_image": mean, "max_image": top, "std_image": ref_std_image(planes, n, region),
            "correlation_image": ref_correlation_image(planes, n, region), "crispness": ref_crispness(mean, region)}


# ------------------------------------------------------------------------- the tests
def test_summary_module_is_exported():
    import kcmc_amd
    from kcmc_amd import summary

    assert kcmc_amd.summary is summary
    for name in ("temporal_sums", "mean_image", "std_image", "correlation_image", "crispness"):
        assert callable(getattr(summary, name)), name
    va = kcmc_amd.VideoAligner
    assert va.SUMMARY_IMAGES is False and va.SUMMARY_NEIGHBOURS == 8
    inst = va()
    for attr in ATTRS:
        assert getattr(inst, attr) is None, attr


ATTRS = ("summary_region", "summary_mean_image", "max_image", "std_image", "correlation_image", "crispness")


def _series_stack(series, H, W, fill=None, seed=0):
    """[F, H, W] uint16 with ``series[(y, x)]`` at the named pixels; the rest random (fill None)
    or constant."""
    F = len(next(iter(series.values())))
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 65536, (F, H, W)).astype(np.uint16) if fill is None else np.full((F, H, W), fill, np.uint16)
    for (y, x), s in series.items():
        st[:, y, x] = s
    return st


def _finish(stack, region, neighbours=8):
    from kcmc_amd import summary

    n, planes, _ = ref_temporal_sums(stack, region, None, neighbours)
    return summary.correlation_image(planes, n, region)


@pytest.mark.parametrize("neighbours", [4, 8])
@pytest.mark.parametrize("region", [(0, 6, 0, 9), (1, 5, 2, 8), (2, 3, 0, 9), (0, 6, 4, 5)])
def test_finishing_functions_equal_the_restatement(neighbours, region):
    from kcmc_amd import summary

    rng = np.random.default_rng(7)
    stack = rng.integers(0, 65536, (37, 6, 9)).astype(np.uint16)
    stack[:, 3, 4] = 777        # a constant pixel
    stack[:, 1, 2] = stack[:, 1, 3]  # two identical series
    n, planes, _ = ref_temporal_sums(stack, region, None, neighbours)
    mean = summary.mean_image(planes, n, region)
    assert mean.dtype == np.uint16
    np.testing.assert_array_equal(mean, ref_mean_image(planes, n, region))
    std = summary.std_image(planes, n, region)
    assert std.dtype == np.float64
    np.testing.assert_array_equal(std, ref_std_image(planes, n, region))
    y0, y1, x0, x1 = region
    np.testing.assert_allclose(std[y0:y1, x0:x1], stack[:, y0:y1, x0:x1].astype(np.float64).std(axis=0), rtol=1e-12)
    corr = summary.correlation_image(planes, n, region)
    assert corr.dtype == np.float64
    np.testing.assert_array_equal(corr, ref_correlation_image(planes, n, region))
    np.testing.assert_array_equal(summary.crispness(mean, region), ref_crispness(mean, region))  # NaN for thin regions


def test_correlation_image_against_corrcoef():
    from kcmc_amd import summary

    rng = np.random.default_rng(12)
    base = rng.integers(0, 40000, (50, 1, 1))
    stack = (base + rng.integers(0, 20000, (50, 5, 7))).astype(np.uint16)  # correlated neighbours
    region = (0, 5, 0, 7)
    for nb in (4, 8):
        n, planes, _ = ref_temporal_sums(stack, region, None, nb)
        got = summary.correlation_image(planes, n, region)
        want = np.zeros((5, 7))
        flat = stack.astype(np.float64)
        for y in range(5):
            for x in range(7):
                rs = [np.corrcoef(flat[:, y, x], flat[:, y + dy, x + dx])[0, 1] for dy, dx in NEIGHBOUR_ORDER[:nb]
                      if 0 <= y + dy < 5 and 0 <= x + dx < 7]
                want[y, x] = np.mean(rs)
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)
        assert got.min() > 0.3


def test_known_answers():
    F = 21
    rng = np.random.default_rng(3)
    s = rng.integers(0, 65536, F).astype(np.uint16)
    # two identical series alone in a 1 x 2 region: r ~ 1; a series and its mirror: r ~ -1
    np.testing.assert_allclose(_finish(_series_stack({(0, 0): s, (0, 1): s}, 1, 2), (0, 1, 0, 2)), [[1.0, 1.0]],
                               rtol=0, atol=1e-15)
    np.testing.assert_allclose(_finish(_series_stack({(0, 0): s, (0, 1): 65535 - s}, 1, 2), (0, 1, 0, 2)),
                               [[-1.0, -1.0]], rtol=0, atol=1e-15)
    # a constant pixel drops out of its neighbours' means, and is NaN itself
    st = _series_stack({(1, 1): np.full(F, 500, np.uint16)}, 3, 3, seed=4)
    for nb in (4, 8):
        got = _finish(st, (0, 3, 0, 3), nb)
        assert math.isnan(got[1, 1])
        n, planes, _ = ref_temporal_sums(st, (0, 3, 0, 3), None, nb)
        flat = st.astype(np.float64)
        rs = [np.corrcoef(flat[:, 0, 0], flat[:, dy, dx])[0, 1] for dy, dx in ((0, 1), (1, 0))]  # (1, 1) left out
        assert got[0, 0] == pytest.approx(np.mean(rs), rel=1e-12)
        if nb == 4:  # the edge pixel (0, 1) keeps right and left only
            rs = [np.corrcoef(flat[:, 0, 1], flat[:, 0, x])[0, 1] for x in (2, 0)]
            assert got[0, 1] == pytest.approx(np.mean(rs), rel=1e-12)
    # a pixel whose neighbours are all constant is NaN (and so are they)
    st = _series_stack({(1, 1): s}, 3, 3, fill=9)
    assert np.isnan(_finish(st, (0, 3, 0, 3))).all()
    # a 1 x 1 region gives all NaN
    st = np.random.default_rng(5).integers(0, 65536, (F, 4, 4)).astype(np.uint16)
    assert np.isnan(_finish(st, (2, 3, 1, 2))).all()


@pytest.mark.parametrize("neighbours,corner,edge,inner", [(8, 3, 5, 8), (4, 2, 3, 4)])
def test_neighbour_counts_at_corners_and_edges(neighbours, corner, edge, inner):
    """A pixel p and one neighbour q carry the series (c, c, 0, 0), every other pixel (c, 0, c, 0):
    r(p, q) is exactly 1 and the covariance of p with every other neighbour exactly 0
    (4 * c^2 - 2c * 2c), so p's value is 1 / (its number of neighbours inside the region)."""
    from kcmc_amd import summary

    H, W = 6, 7
    region = y0, y1, x0, x1 = (1, 5, 1, 6)  # 4 x 5 inside a larger image
    s1, s2 = np.array([1000, 1000, 0, 0], np.uint16), np.array([1000, 0, 1000, 0], np.uint16)

    def value(p, q):
        st = np.broadcast_to(s2[:, None, None], (4, H, W)).copy()
        st[:, p[0], p[1]] = s1
        st[:, q[0], q[1]] = s1
        n, planes, _ = ref_temporal_sums(st, region, None, neighbours)
        got = summary.correlation_image(planes, n, region)
        np.testing.assert_array_equal(got, ref_correlation_image(planes, n, region))
        assert all(np.isnan(border).all() for border in (got[0], got[:, 0], got[5], got[:, 6]))
        return got[p]

    for p, q in (((y0, x0), (y0, x0 + 1)), ((y0, x1 - 1), (y0 + 1, x1 - 1)), ((y1 - 1, x0), (y1 - 1, x0 + 1)),
                 ((y1 - 1, x1 - 1), (y1 - 2, x1 - 1))):
        assert value(p, q) == 1.0 / corner, (p, q)
    for p, q in (((y0, x0 + 1), (y0, x0 + 2)), ((y0 + 1, x0), (y0 + 2, x0)), ((y1 - 1, x0 + 2), (y1 - 1, x0 + 1)),
                 ((y0 + 2, x1 - 1), (y0 + 1, x1 - 1))):
        assert value(p, q) == 1.0 / edge, (p, q)
    for q in ((y0 + 1, x0 + 2), (y0 + 2, x0 + 1), (y0 + 1, x0), (y0, x0 + 1)):
        assert value((y0 + 1, x0 + 1), q) == 1.0 / inner, q


@pytest.mark.parametrize("neighbours", [4, 8])
def test_int64_path_equals_python_int_path(neighbours):
    from kcmc_amd import summary

    rng = np.random.default_rng(21)
    stack = rng.integers(0, 65536, (37, 6, 9)).astype(np.uint16)
    region = (0, 6, 1, 9)
    n, planes, _ = ref_temporal_sums(stack, region, None, neighbours)
    assert n * int(planes[1].max()) < 1 << 63
    as_ints = planes.astype(object)  # the same planes; the module decides by their values ...
    for fn in (summary.mean_image, summary.std_image, summary.correlation_image):
        np.testing.assert_array_equal(fn(as_ints, n, region), fn(planes, n, region))
    # ... so force the Python-int arithmetic and compare bit for bit
    forced = {}
    real = summary._planes

    def python_ints(p, n_, region_):
        cut, n_, shape, region_ = real(p, n_, region_)
        forced["seen"] = True
        return cut.astype(object), n_, shape, region_

    summary._planes = python_ints
    try:
        slow = [fn(planes, n, region) for fn in (summary.mean_image, summary.std_image, summary.correlation_image)]
    finally:
        summary._planes = real
    assert forced["seen"]
    for got, fn in zip(slow, (summary.mean_image, summary.std_image, summary.correlation_image)):
        np.testing.assert_array_equal(got, fn(planes, n, region))
    np.testing.assert_array_equal(slow[2], ref_correlation_image(planes, n, region))


def test_switch_to_python_ints_is_exactly_at_2_to_63():
    """n frames of 65535 at a pixel: S1 = n * 65535^2, and n * S1 reaches 2^63 between
    n = 46341 and n = 46342 ((2^63)^(1/2) / 65535 = 46341.6...)."""
    from kcmc_amd import summary

    v = 65535
    assert 46341 ** 2 * v * v < 1 << 63 <= 46342 ** 2 * v * v
    region = (0, 1, 0, 3)
    for n, big in ((46341, False), (46342, True)):
        # pixel 0: all 65535; pixel 1: half 65535 and half 0 (n even or odd: floor); pixel 2: all 65535
        k = n // 2
        planes = np.zeros((4, 1, 3), np.int64)
        planes[0, 0] = [n * v, k * v, n * v]
        planes[1, 0] = [n * v * v, k * v * v, n * v * v]
        planes[2, 0] = [k * v * v, k * v * v, 0]
        cut = summary._planes(planes, n, region)[0]
        assert (cut.dtype == object) == big, (n, cut.dtype)
        np.testing.assert_array_equal(summary.mean_image(planes, n, region), [[v, (k * v + n // 2) // n, v]])
        std = summary.std_image(planes, n, region)
        assert std[0, 0] == 0.0 and std[0, 2] == 0.0
        assert std[0, 1] == math.sqrt(float(n * k * v * v - k * k * v * v)) / n
        np.testing.assert_array_equal(std, ref_std_image(planes, n, region))
        corr = summary.correlation_image(planes, n, region)
        assert np.isnan(corr).all()  # the varying pixel's neighbours are constant
        np.testing.assert_array_equal(corr, ref_correlation_image(planes, n, region))
    # beyond the switch, with two varying pixels: what wrapped int64 arithmetic cannot give
    n = 70000
    k = n // 2
    planes = np.zeros((4, 1, 2), np.int64)
    planes[0, 0] = [k * v, k * v]            # both pixels: the first k frames 65535, the rest 0
    planes[1, 0] = [k * v * v, k * v * v]
    planes[2, 0] = [k * v * v, 0]
    assert n * k * v * v >= 1 << 63
    corr = summary.correlation_image(planes, n, (0, 1, 0, 2))
    np.testing.assert_array_equal(corr, ref_correlation_image(planes, n, (0, 1, 0, 2)))
    np.testing.assert_allclose(corr, [[1.0, 1.0]], rtol=0, atol=1e-15)


def test_crispness():
    from kcmc_amd import summary

    H, W = 7, 9
    ys, xs = np.mgrid[0:H, 0:W]
    ramp = (100 + 3 * xs + 5 * ys).astype(np.uint16)  # gx = 6, gy = 10 everywhere
    region = (0, H, 0, W)
    assert summary.crispness(ramp, region) == math.sqrt(float((H - 2) * (W - 2) * (36 + 100))) / 2
    assert summary.crispness(ramp, (1, 6, 2, 8)) == math.sqrt(float(3 * 4 * 136)) / 2
    gy, gx = np.gradient(ramp.astype(np.float64))
    assert summary.crispness(ramp, region) == pytest.approx(
        np.linalg.norm(np.hypot(gx, gy)[1:-1, 1:-1]), rel=1e-14)
    assert summary.crispness(np.full((H, W), 4321, np.uint16), region) == 0.0
    for empty in ((0, 2, 0, W), (0, H, 3, 5), (2, 3, 4, 5)):
        assert math.isnan(summary.crispness(ramp, empty))
    rng = np.random.default_rng(9)
    m = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    assert summary.crispness(m, (1, 7, 0, 8)) == ref_crispness(m, (1, 7, 0, 8))


def test_finishing_functions_reject_bad_arguments():
    from kcmc_amd import summary

    planes = np.zeros((6, 4, 5), np.int64)
    for fn in (summary.mean_image, summary.std_image, summary.correlation_image):
        with pytest.raises(ValueError):
            fn(planes, 0, (0, 4, 0, 5))        # no frame
        with pytest.raises(ValueError):
            fn(planes, 3, (2, 2, 0, 5))        # empty
        with pytest.raises(ValueError):
            fn(planes, 3, (0, 5, 0, 5))        # outside
        with pytest.raises(ValueError):
            fn(planes[:5], 3, (0, 4, 0, 5))    # neither 4 nor 6 planes
    for bad in (6, 0, True, "8"):
        with pytest.raises(ValueError):
            summary.check_neighbours(bad)


def test_restatement_of_the_planes():
    """The restatement itself on a stack small enough to read: a 2 x 3 image, rectangle columns
    [0, 2): column 1 has no right partner inside, and never pairs with column 0 of the next row."""
    st = np.array([[[1, 2, 9], [3, 4, 9]], [[5, 6, 9], [7, 8, 9]]], np.uint16)
    n, planes, top = ref_temporal_sums(st, (0, 2, 0, 2), None, 8)
    assert n == 2
    np.testing.assert_array_equal(planes[0], [[6, 8, 0], [10, 12, 0]])
    np.testing.assert_array_equal(planes[1], [[26, 40, 0], [58, 80, 0]])
    np.testing.assert_array_equal(planes[2], [[1 * 2 + 5 * 6, 0, 0], [3 * 4 + 7 * 8, 0, 0]])      # right
    np.testing.assert_array_equal(planes[3], [[1 * 3 + 5 * 7, 2 * 4 + 6 * 8, 0], [0, 0, 0]])      # down
    np.testing.assert_array_equal(planes[4], [[1 * 4 + 5 * 8, 0, 0], [0, 0, 0]])                  # down-right
    np.testing.assert_array_equal(planes[5], [[0, 2 * 3 + 6 * 7, 0], [0, 0, 0]])                  # down-left
    np.testing.assert_array_equal(top, [[5, 6, 0], [7, 8, 0]])
    n, planes, top = ref_temporal_sums(st, (0, 2, 0, 2), [False, True], 4)
    assert n == 1 and planes.shape == (4, 2, 3)
    np.testing.assert_array_equal(planes[2], [[30, 0, 0], [56, 0, 0]])
    n, planes, top = ref_temporal_sums(st, (0, 2, 0, 3), [False, False], 8)
    assert n == 0 and not planes.any() and not top.any()


# ------------------------------------------------------------------ the C entry and the ABI
def test_header_binding_and_abi():
    import os
    import re

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    decl = re.search(r"int\s+kcmc_temporal_sums_u16\s*\(([^)]*)\)\s*;", src)
    assert decl, "include/kcmc.h does not declare kcmc_temporal_sums_u16"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["kcmc_ctx* ctx", "const uint16_t* frames_dev", "int n_frames", "int H", "int W",
                    "const uint8_t* sel_dev", "int y0", "int y1", "int x0", "int x1", "int neighbours",
                    "long long* out_sums_dev", "uint16_t* out_max_dev", "kcmc_stream_t stream"]
    assert "kcmc_temporal_sums_u16" in _lib.EXPORTED_SYMBOLS
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES["kcmc_temporal_sums_u16"] == ([P, P, I, I, I, P, I, I, I, I, I, P, P, P], I)
    assert _lib.ABI_VERSION == 2 and _lib.load().kcmc_abi_version() == 2
    from kcmc_amd import build

    assert "temporal_sums.hip" in build.SOURCES


def test_entry_point_validates_before_touching_the_gpu():
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(256, np.int64)
    p = buf.ctypes.data_as(P)
    fake_ctx = P(buf.ctypes.data)  # never dereferenced: the argument checks come first
    EINVAL = _lib.KCMC_EINVAL
    fn = L.kcmc_temporal_sums_u16
    assert fn(None, p, 1, 4, 4, None, 0, 4, 0, 4, 8, p, p, None) == EINVAL
    assert b"ctx" in L.kcmc_last_error()
    assert fn(fake_ctx, None, 1, 4, 4, None, 0, 4, 0, 4, 8, p, p, None) == EINVAL
    assert b"NULL" in L.kcmc_last_error()
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, 8, None, p, None) == EINVAL
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, 8, p, None, None) == EINVAL
    assert fn(fake_ctx, p, 0, 4, 4, None, 0, 4, 0, 4, 8, None, p, None) == EINVAL  # outputs also without frames
    assert fn(fake_ctx, p, 1, 4, 4, None, 2, 2, 0, 4, 8, p, p, None) == EINVAL  # empty
    assert b"empty" in L.kcmc_last_error()
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 3, 1, 8, p, p, None) == EINVAL
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 5, 0, 4, 8, p, p, None) == EINVAL  # outside
    assert b"outside" in L.kcmc_last_error()
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, -1, 4, 8, p, p, None) == EINVAL
    assert fn(fake_ctx, p, 1, 1 << 16, 1 << 15, None, 0, 4, 0, 4, 8, p, p, None) == EINVAL
    assert b"2^31" in L.kcmc_last_error()
    assert fn(fake_ctx, p, -1, 4, 4, None, 0, 4, 0, 4, 8, p, p, None) == EINVAL
    for nb in (6, 0, -8, 16):
        assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, nb, p, p, None) == EINVAL, nb
        assert b"neighbours" in L.kcmc_last_error()
    odd = P(buf.ctypes.data + 2)
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, 8, p, odd, None) == EINVAL  # max image not 4-byte aligned
    assert fn(fake_ctx, p, 1, 4, 4, None, 0, 4, 0, 4, 8, P(buf.ctypes.data + 4), p, None) == EINVAL  # planes not 8-byte


def test_switch_checks_fail_before_any_work():
    """The unsupported combinations raise from the public entry points before they look at
    their inputs (no GPU is touched)."""
    from kcmc_amd import VideoAligner

    class Proj(VideoAligner):
        RANSAC_MODEL = "projective"
        SUMMARY_IMAGES = True

    class Piecewise(VideoAligner):
        PIECEWISE_GRID = (2, 2)
        SUMMARY_IMAGES = True

    class Field(VideoAligner):
        REFINE = "intensity"
        REFINE_GRID = (2, 2)
        SUMMARY_IMAGES = True

    class Six(VideoAligner):
        SUMMARY_IMAGES = True
        SUMMARY_NEIGHBOURS = 6

    for cls in (Proj, Piecewise, Field):
        with pytest.raises(NotImplementedError, match="SUMMARY_IMAGES"):
            cls().align_images(None, 10, "orb", 30)
        with pytest.raises(NotImplementedError, match="SUMMARY_IMAGES"):
            cls().align_keypoints(None, None, None, None, None, 10)
    with pytest.raises(ValueError, match="SUMMARY_NEIGHBOURS"):
        Six().align_images(None, 10, "orb", 30)
    with pytest.raises(ValueError, match="SUMMARY_NEIGHBOURS"):
        Six().align_keypoints(None, None, None, None, None, 10)

    class Colour(VideoAligner):
        SUMMARY_IMAGES = True

    with pytest.raises(NotImplementedError, match="grayscale"):
        Colour().align_images(np.zeros((2, 8, 8, 3), np.uint16), 10, "orb", 30)
    va = Colour()
    va.crispness = 1.0  # a stale result of an earlier call is reset before the checks of the next
    with pytest.raises(NotImplementedError):
        va.align_images(np.zeros((2, 8, 8, 3), np.uint16), 10, "orb", 30)
    assert all(getattr(va, a) is None for a in ATTRS)
