"""The box band-pass prefilter (kcmc_amd.prefilter, csrc/band_filter.hip) restated in numpy
(ref_box_bandpass), the restatement pinned by a brute-force loop over windows, the two properties
that follow from the definition, the checks of the radii and of the VideoAligner switch, the ABI
and its validation -- all without a GPU -- and the filter's effect on the CPU oracle chain for a
one-photon-like scene.  tests/test_gpu_prefilter.py holds the kernel to the restatement bit for
bit.

Build-defined semantics (include/kcmc.h): for a radius rho the window of (y, x) is
rows max(0, y - rho) .. min(H - 1, y + rho) and the columns likewise, n its pixel count, S its sum,
m_rho = (S + n // 2) // n; dst = max(m_s - (m_r if r > 0 else 0), 0)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle
from kcmc_amd import _lib, orb, prefilter
from test_orb_host import detect_oracle

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")


# ------------------------------------------------------------------------ the restatement
def _rounded_box_mean(a, rho):
    """m_rho of one int64 frame from its integral image."""
    if rho == 0:
        return a
    H, W = a.shape
    I = np.zeros((H + 1, W + 1), np.int64)
    I[1:, 1:] = a.cumsum(0).cumsum(1)
    y0, y1 = np.maximum(0, np.arange(H) - rho), np.minimum(H - 1, np.arange(H) + rho) + 1
    x0, x1 = np.maximum(0, np.arange(W) - rho), np.minimum(W - 1, np.arange(W) + rho) + 1
    S = I[y1][:, x1] - I[y0][:, x1] - I[y1][:, x0] + I[y0][:, x0]
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return (S + n // 2) // n


def ref_box_bandpass(x, s, r):
    """The definition for a frame [H, W] or a stack [F, H, W] of uint16; uint16 of the same shape."""
    x = np.asarray(x)
    assert x.dtype == np.uint16 and x.ndim in (2, 3)
    if x.ndim == 3:
        return np.stack([ref_box_bandpass(f, s, r) for f in x]) if len(x) else x.copy()
    a = x.astype(np.int64)
    m = _rounded_box_mean(a, s) - (_rounded_box_mean(a, r) if r > 0 else 0)
    return np.maximum(m, 0).astype(np.uint16)


def brute_box_bandpass(x, s, r):
    """The same, window by window in Python integers."""
    H, W = x.shape
    out = np.zeros((H, W), np.uint16)

    def mean(y, xx, rho):
        win = x[max(0, y - rho):min(H - 1, y + rho) + 1, max(0, xx - rho):min(W - 1, xx + rho) + 1]
        n, S = win.size, sum(int(v) for v in win.reshape(-1))
        return (S + n // 2) // n

    for y in range(H):
        for xx in range(W):
            out[y, xx] = max(mean(y, xx, s) - (mean(y, xx, r) if r > 0 else 0), 0)
    return out


def random_u16(shape, seed):
    return np.random.default_rng(seed).integers(0, 65536, shape).astype(np.uint16)


RADII = [(0, 1), (4, 5), (4, 32), (0, 32), (1, 0), (4, 0), (2, 12)]


@pytest.mark.parametrize("H,W", [(1, 1), (3, 9), (7, 5), (12, 13)])
def test_restatement_is_the_definition(H, W):
    x = random_u16((H, W), 100 * H + W)
    x[H // 2, W // 2] = 65535
    for s, r in RADII + [(1, 2), (0, 3)]:
        np.testing.assert_array_equal(ref_box_bandpass(x, s, r), brute_box_bandpass(x, s, r), err_msg=f"{s} {r}")
    np.testing.assert_array_equal(ref_box_bandpass(np.stack([x, x[::-1]]), 1, 3)[1], brute_box_bandpass(x[::-1], 1, 3))
    assert ref_box_bandpass(np.zeros((0, H, W), np.uint16), 1, 3).shape == (0, H, W)


def test_known_answers():
    x = np.array([[0, 0, 0], [0, 9, 0], [0, 0, 0]], np.uint16)
    # s = 1: the corner windows hold 4 pixels, the edge windows 6, the centre's 9
    np.testing.assert_array_equal(ref_box_bandpass(x, 1, 0), [[2, 2, 2], [2, 1, 2], [2, 2, 2]])  # (9 + n // 2) // n
    np.testing.assert_array_equal(ref_box_bandpass(x, 0, 1), [[0, 0, 0], [0, 8, 0], [0, 0, 0]])
    half = np.array([[65535, 0]], np.uint16)  # the mean of two is 32767.5: rounds up
    np.testing.assert_array_equal(ref_box_bandpass(half, 1, 0), [[32768, 32768]])


@pytest.mark.parametrize("c", [0, 1, 777, 65535])
def test_a_constant_frame_filters_to_zero_or_to_itself(c):
    x = np.full((2, 9, 70), c, np.uint16)
    for s, r in RADII:
        want = 0 if r > 0 else c
        assert (ref_box_bandpass(x, s, r) == want).all(), (s, r)


def test_a_background_wider_than_the_frame_is_the_frame_mean():
    x = random_u16((9, 12), 4)
    n, S = x.size, int(x.astype(np.int64).sum())
    mean = (S + n // 2) // n
    for r in (11, 12, 32):  # r >= max(H, W) - 1
        np.testing.assert_array_equal(ref_box_bandpass(x, 0, r), np.maximum(x.astype(np.int64) - mean, 0))
    assert (ref_box_bandpass(x, 0, 10) != ref_box_bandpass(x, 0, 11)).any()


# ------------------------------------------------------------------------------ the radii
def test_check_radii():
    assert prefilter.check_radii(1, 12) == (1, 12) and prefilter.check_radii(0, 1) == (0, 1)
    assert prefilter.check_radii(4, 0) == (4, 0) and prefilter.check_radii(np.int64(4), np.int32(32)) == (4, 32)
    assert isinstance(prefilter.check_radii(np.int64(2), 3)[0], int)
    for s, r in [(0, 0), (-1, 3), (5, 9), (1, 33), (1, -1), (2, 2), (3, 1), (4, 4), (True, 3), (1, True), (1.0, 3),
                 (1, 3.0), ("1", 3), (None, 3), (1, None)]:
        with pytest.raises(ValueError):
            prefilter.check_radii(s, r)


# ------------------------------------------------------------------ how the kernel cuts a call
def test_launch_plan_has_no_empty_chunk():
    """(strip columns, strips, chunks, rows per chunk) from the library itself.  Every chunk holds a
    row -- (chunks - 1) rows < H <= chunks rows -- at every height: a cut by ceil(H / min(want, H // 32))
    alone leaves trailing chunks empty at tall frames (2160 rows in 67 chunks of 33 end at 2211), and
    a workgroup of an empty chunk would start beyond its frame."""
    assert prefilter.launch_plan(2000, 1080, 1920, 1, 12) == (232, 9, 1, 1080)   # enough strips: whole frames
    assert prefilter.launch_plan(2000, 1080, 1920, 4, 32) == (192, 10, 1, 1080)
    assert prefilter.launch_plan(1, 64, 500, 3, 0) == (250, 2, 2, 32)            # a few frames: chunks of >= 32 rows
    assert prefilter.launch_plan(1, 63, 500, 3, 0)[2:] == (1, 63)
    assert prefilter.launch_plan(1, 2160, 1920, 1, 12)[2:] == (66, 33)
    assert prefilter.launch_plan(0, 5, 5, 1, 0) == (254, 1, 1, 5)                # an empty call has a plan too
    heights = list(range(1, 1400)) + list(range(1400, 9000, 7)) + [2050, 2160, 4320, 32767, 100000]
    for s, r in RADII:
        for n_frames, W in ((1, 40), (1, 1920), (3, 700), (40, 300)):
            for H in heights:
                tw, strips, chunks, rows = prefilter.launch_plan(n_frames, H, W, s, r)
                assert tw == 256 - 2 * max(s, r) and strips == -(-W // tw)
                assert chunks >= 1 and (chunks - 1) * rows < H <= chunks * rows, (n_frames, H, W, s, r)
                assert chunks == 1 or rows >= 32
    for bad in (dict(H=0), dict(W=0), dict(n_frames=-1)):
        with pytest.raises(ValueError):
            prefilter.launch_plan(**{**dict(n_frames=1, H=5, W=5, smooth=1, background=0), **bad})
    with pytest.raises(ValueError):
        prefilter.launch_plan(1, 5, 5, 0, 0)
    assert _lib.load().kcmc_box_bandpass_plan(1, 5, 5, 1, 0, None) == _lib.KCMC_EINVAL


# ------------------------------------------------------------------------------ the divide
def test_reciprocal_divide_is_exact_at_every_window_size():
    """The kernel's rounded mean (csrc/band_filter.hip, rounded_mean) restated in float32: q =
    trunc(float(a) * inv) with a = S + n // 2, corrected once by the signed remainder a - q n.  For every
    n a clipped window can have (1299 products of two counts in 1 .. 65), at both ends of every
    quotient 0 .. 65535, with inv the rounded reciprocal and one ulp off either way (the hardware
    reciprocal is good to one ulp): the exact quotient."""
    ns = sorted({a * b for a in range(1, 66) for b in range(1, 66)})
    assert len(ns) == 1299
    q = np.arange(65536, dtype=np.uint32)
    for n in ns:
        inv0 = np.float32(1.0) / np.float32(n)
        lo = q * np.uint32(n)
        a = np.concatenate([lo, lo + np.uint32(n - 1)])
        a = a[a <= 65535 * n + n // 2]  # S <= 65535 n
        for inv in (inv0, np.nextafter(inv0, np.float32(0)), np.nextafter(inv0, np.float32(1))):
            g = (a.astype(np.float32) * inv).astype(np.uint32)
            rem = (a - g * np.uint32(n)).astype(np.int32)
            g = np.where(rem < 0, g - 1, np.where(rem >= n, g + 1, g))
            assert (g == a // n).all(), n


def test_package_exports_the_module():
    import kcmc_amd

    assert kcmc_amd.prefilter is prefilter and "prefilter" in kcmc_amd.__all__


# ------------------------------------------------------------------ the switch without a GPU
def _va(**kw):
    from kcmc_amd import VideoAligner

    return type("VA", (VideoAligner,), kw)()


def test_switch_defaults_and_results():
    from kcmc_amd import VideoAligner

    assert (VideoAligner.DETECT_SMOOTH_RADIUS, VideoAligner.DETECT_BACKGROUND_RADIUS) == (0, 0)
    va = VideoAligner()
    assert va.prefilter_radii is None and va.prefilter_brightest_px is None
    assert va._prefilter_on() is None
    assert _va(DETECT_SMOOTH_RADIUS=1, DETECT_BACKGROUND_RADIUS=12)._prefilter_on() == (1, 12)
    assert _va(DETECT_SMOOTH_RADIUS=2)._prefilter_on() == (2, 0)
    assert _va(DETECT_BACKGROUND_RADIUS=np.int64(8))._prefilter_on() == (0, 8)


def test_switch_checks_fail_before_any_work():
    stack4 = np.zeros((2, 4, 4, 3), np.uint16)
    bad = [dict(DETECT_SMOOTH_RADIUS=5), dict(DETECT_SMOOTH_RADIUS=-1), dict(DETECT_SMOOTH_RADIUS=True),
           dict(DETECT_SMOOTH_RADIUS=1.0), dict(DETECT_BACKGROUND_RADIUS=33), dict(DETECT_BACKGROUND_RADIUS=-2),
           dict(DETECT_BACKGROUND_RADIUS="8"), dict(DETECT_SMOOTH_RADIUS=None),
           dict(DETECT_SMOOTH_RADIUS=2, DETECT_BACKGROUND_RADIUS=2),   # r <= s
           dict(DETECT_SMOOTH_RADIUS=4, DETECT_BACKGROUND_RADIUS=1)]
    cases = [(kw, ValueError, "DETECT_SMOOTH_RADIUS / DETECT_BACKGROUND_RADIUS", None) for kw in bad]
    cases += [(dict(DETECT_SMOOTH_RADIUS=1, DETECT_BACKGROUND_RADIUS=12), NotImplementedError, "grayscale", stack4),
              (dict(DETECT_SMOOTH_RADIUS=2), NotImplementedError, "grayscale", stack4)]
    for kw, err, match, images in cases:
        va = _va(**kw)
        va.prefilter_radii, va.prefilter_brightest_px = (1, 2), 5.0  # stale results: reset by every call
        with pytest.raises(err, match=match):
            va.align_images(images, 10, "orb", 30)
        assert va.prefilter_radii is None and va.prefilter_brightest_px is None
        with pytest.raises(err, match=match):
            _va(**kw).align_keypoints(images, None, None, None, None, 10)


# -------------------------------------------------------------------------------- the ABI
def test_header_and_binding_table_name_the_entry_point():
    with open(HEADER) as f:
        header = f.read()
    name = "kcmc_box_bandpass_u16"
    assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES
    assert f"int {name}(" in header
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _lib._SIGNATURES[name] == ([P, P, P, I, I, I, I, I, P], I)
    assert "#define KCMC_ABI_VERSION 2" in header and _lib.ABI_VERSION == 2
    assert _lib.load().kcmc_abi_version() == 2


def check_validation(ctx, good):
    """Every contract violation is KCMC_EINVAL before any device work.  ``ctx``: a context handle
    (never dereferenced by the checks); ``good``: device pointers (src, dst) of valid 2 x 33 x 40
    calls, or None on a box without a GPU (a host buffer stands in: nothing reads it)."""
    L = _lib.load()
    P = ctypes.c_void_p
    buf = np.zeros(8192, np.uint16)
    src, dst = good if good is not None else (buf.ctypes.data, buf.ctypes.data + 2 * 2 * 33 * 40)
    p = lambda v: None if v is None else P(v)  # noqa: E731
    E, OK = _lib.KCMC_EINVAL, _lib.KCMC_OK
    n = 2 * 33 * 40

    def call(ctx=ctx, src=src, dst=dst, n_frames=2, H=33, W=40, s=1, r=12):
        return L.kcmc_box_bandpass_u16(ctx, p(src), p(dst), n_frames, H, W, s, r, None)

    assert call(ctx=None) == E and b"ctx" in L.kcmc_last_error()
    assert call(src=None) == E and b"NULL" in L.kcmc_last_error()
    assert call(dst=None) == E and b"NULL" in L.kcmc_last_error()
    assert call(n_frames=-1) == E and b"n_frames" in L.kcmc_last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(W=-1)):
        assert call(**kw) == E and b"H and W" in L.kcmc_last_error(), kw
    for s in (-1, 5):
        assert call(s=s) == E and b"smooth_radius" in L.kcmc_last_error(), s
    for r in (-1, 33):
        assert call(r=r) == E and b"background_radius" in L.kcmc_last_error(), r
    assert call(s=0, r=0) == E and b"both 0" in L.kcmc_last_error()
    for s, r in ((1, 1), (4, 2), (4, 4), (2, 1)):  # 0 < r <= s
        assert call(s=s, r=r) == E and b"exceed smooth_radius" in L.kcmc_last_error(), (s, r)
    for delta in (0, 2, -2, 2 * (n - 1), -2 * (n - 1)):  # the same stack, and partial overlap either way round
        assert call(dst=src + delta) == E and b"overlap" in L.kcmc_last_error(), delta
    assert call(n_frames=0) == OK and call(n_frames=0, src=None, dst=None) == OK
    assert call(n_frames=0, s=0, r=0) == E  # the radii are checked also for an empty call
    if good is not None:
        assert call() == OK and call(s=4, r=0) == OK and call(s=0, r=32) == OK


def test_entry_point_validates_before_touching_the_gpu():
    check_validation(ctypes.c_void_p(np.zeros(8, np.int64).ctypes.data), None)


# ------------------------------------------------------- the effect, on the CPU oracle chain
SCENE_H, SCENE_W = 240, 320
SCENE_SHIFT = (5, -3)  # (dx, dy) of the second frame's content against the first's, px
N_KP_FRAME_SKIP = 3
EFFECT_RADII = (1, 12)


@functools.lru_cache(maxsize=1)
def one_photon_pair(seed=12):
    """Two uint16 frames [2, 240, 320] of one one-photon-like scene, the second moved by SCENE_SHIFT:
    Gaussian blobs (sigma 1.5 .. 3 px) of 300 .. 2000 grey levels on a vignetted background that peaks
    at 30000, with Poisson-like noise (sigma = sqrt(signal) / 2, drawn per frame)."""
    rng = np.random.default_rng(seed)
    m = 16
    Hs, Ws = SCENE_H + 2 * m, SCENE_W + 2 * m
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    cells = np.zeros((Hs, Ws))
    for _ in range(120):
        cy, cx = rng.uniform(0, Hs), rng.uniform(0, Ws)
        sig, amp = rng.uniform(1.5, 3.0), rng.uniform(300, 2000)
        cells += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig))
    y, x = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)
    rad2 = ((y - (SCENE_H - 1) / 2) / SCENE_H) ** 2 + ((x - (SCENE_W - 1) / 2) / SCENE_W) ** 2
    background = 30000.0 * (1.0 - 1.2 * rad2)  # fixed to the sensor: the vignette does not move
    frames = []
    for k, (dx, dy) in enumerate(((0, 0), SCENE_SHIFT)):
        signal = background + cells[m - dy:m - dy + SCENE_H, m - dx:m - dx + SCENE_W]
        noise = np.random.default_rng([seed, k]).normal(0, 1, signal.shape) * np.sqrt(signal) / 2
        frames.append(np.clip(np.rint(signal + noise), 0, 65535).astype(np.uint16))
    return np.stack(frames)


def max_scale_u8(stack_u16):
    """VA:479-492 on the host: the stack scaled by its 99.99th percentile to uint8."""
    b = np.percentile(stack_u16, 99.99)
    return np.clip(stack_u16 / b * 255, 0, 255).astype(np.uint8)


def oracle_chain(tpl_u8, frm_u8, p=None):
    """detect -> knn (template descriptors as queries) -> ratio 0.75 -> rigid RANSAC, the chain of
    tests/test_orb_pyramid_host.py with the single-level detector and the rigid model:
    (n_ratio_matches, n_inliers, params [2, 3] frame -> template)."""
    p = p or orb.OrbParams()
    kt, dt = detect_oracle(tpl_u8, p)
    kf, df = detect_oracle(frm_u8, p)
    if len(kt) < 2 or len(kf) < 2:
        return 0, 0, np.full((2, 3), np.nan)
    idx, dist = oracle.knn2_l2u8(dt, df)
    keep = dist[:, 0] < 0.75 * dist[:, 1]
    if keep.sum() < 2:
        return int(keep.sum()), 0, np.full((2, 3), np.nan)
    src, dst = kf[idx[keep, 0]], kt[keep]
    params, _, _, n_in = oracle.ransac_rigid(src, dst)
    return int(keep.sum()), n_in, params


def test_the_filter_gives_the_chain_its_keypoints_on_a_one_photon_scene():
    """Cells of 300 .. 2000 grey levels on a vignette of 30000, the second frame moved by (5, -3) px.
    Scaled by the 99.99th percentile as they are, the frames give the detector nothing: 0 ratio
    matches, no model.  After the (1, 12) band-pass the chain finds 23 ratio matches and 18 RANSAC
    inliers and recovers the translation to 0.067 px (measured on the oracle; over the seeds 11 .. 14:
    12 .. 29 matches, 6 .. 18 inliers, 0.07 .. 0.33 px).  The tolerance is twice the measured error,
    0.14 px."""
    raw = one_photon_pair()
    n_ratio0, n_in0, params0 = oracle_chain(*max_scale_u8(raw))
    n_ratio1, n_in1, params1 = oracle_chain(*max_scale_u8(ref_box_bandpass(raw, *EFFECT_RADII)))
    dx, dy = SCENE_SHIFT
    err1 = np.hypot(params1[0, 2] + dx, params1[1, 2] + dy)  # frame -> template undoes the shift
    err0 = np.hypot(params0[0, 2] + dx, params0[1, 2] + dy)
    print("raw:", n_ratio0, n_in0, err0, "filtered:", n_ratio1, n_in1, err1, params1.tolist())
    assert n_in0 < N_KP_FRAME_SKIP or not err0 <= 1.0   # the premise: the plain chain fails
    assert n_ratio1 > n_ratio0 and n_in1 > n_in0
    assert n_in1 >= N_KP_FRAME_SKIP
    assert err1 <= 0.14
