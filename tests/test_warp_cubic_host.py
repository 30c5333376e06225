"""The bicubic warp on the host: the numpy restatement ``ref_warp_affine_cubic`` of the
build-defined INTER_CUBIC semantics (include/kcmc.h; the yardstick of
tests/test_gpu_warp_cubic.py), its weight table, known answers, the accuracy claim against the
bilinear warp, quality.valid_region(taps=4), and the switch's plumbing and refusals.  Parity with
cv2 is unpinned: this file pins the definition."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle
from kcmc_amd import VideoAligner, _lib, pipeline, quality, stages

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kcmc.h")
F32 = np.float32


# ------------------------------------------------------------------ the restatement
def cubic_weights_f32(f):
    """OpenCV's interpolateCubic at t = f / 32, operation by operation in float32."""
    A, t = F32(-0.75), F32(f) * F32(1.0 / 32.0)
    one = F32(1)
    c0 = ((A * (t + one) - F32(5) * A) * (t + one) + F32(8) * A) * (t + one) - F32(4) * A
    c1 = ((A + F32(2)) * t - (A + F32(3))) * t * t + one
    u = one - t
    c2 = ((A + F32(2)) * u - (A + F32(3))) * u * u + one
    c3 = one - c0 - c1 - c2
    out = np.array([c0, c1, c2, c3])
    assert out.dtype == np.float32
    return out


def cubic_weights_exact(f):
    A, t = Fraction(-3, 4), Fraction(f, 32)
    c0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
    c1 = ((A + 2) * t - (A + 3)) * t * t + 1
    u = 1 - t
    c2 = ((A + 2) * u - (A + 3)) * u * u + 1
    return [c0, c1, c2, 1 - c0 - c1 - c2]


CUBIC_TAB = np.stack([cubic_weights_f32(f) for f in range(32)])  # [32, 4] float32


def _invert(M):
    """OpenCV warpAffine's in-place inversion, operation by operation."""
    M = np.array(M, np.float64).reshape(6)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def fixed_point_coords(M, H, W, inverse_map=False):
    """(X, Y) [H, W] int64 in 1/1024 px: WarpAffineInvoker's integer arithmetic, as the linear
    restatements (tests/test_piecewise_host.py) and the oracle build it.  None for a NaN map."""
    if np.isnan(np.asarray(M, np.float64)).any():
        return None
    m = np.asarray(M, np.float64).reshape(6) if inverse_map else _invert(M)
    if np.isnan(m).any():
        return None
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    adelta = np.rint(m[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * x * 1024).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024).astype(np.int64) + 16
    return X0[:, None] + adelta[None, :], Y0[:, None] + bdelta[None, :]


def interior_mask(M, H, W, inverse_map=False):
    """[H, W] bool: the pixels whose whole 4 x 4 footprint is inside the image."""
    XY = fixed_point_coords(M, H, W, inverse_map)
    if XY is None:
        return np.zeros((H, W), bool)
    sx, sy = np.clip(XY[0] >> 10, -32768, 32767), np.clip(XY[1] >> 10, -32768, 32767)
    return (sx - 1 >= 0) & (sx + 2 <= W - 1) & (sy - 1 >= 0) & (sy + 2 <= H - 1)


def ref_warp_affine_cubic(src, M, inverse_map=False):
    """The definition for one frame src [H, W] u16 and one 2 x 3 map, or for frames [F, H, W]
    and maps [F, 2, 3]."""
    src = np.asarray(src)
    if src.ndim == 3:
        M = np.asarray(M, np.float64)
        return np.stack([ref_warp_affine_cubic(src[f], M[f], inverse_map) for f in range(src.shape[0])])
    assert src.dtype == np.uint16 and src.ndim == 2
    H, W = src.shape
    XY = fixed_point_coords(M, H, W, inverse_map)
    if XY is None:
        return np.zeros((H, W), np.uint16)
    X, Y = XY
    sx, sy = np.clip(X >> 10, -32768, 32767), np.clip(Y >> 10, -32768, 32767)
    cx, cy = CUBIC_TAB[(X >> 5) & 31], CUBIC_TAB[(Y >> 5) & 31]  # [H, W, 4] float32
    p = np.empty((4, 4, H, W), np.float32)
    for i in range(4):
        for j in range(4):
            yy, xx = sy - 1 + i, sx - 1 + j
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tap = np.where(ok, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0).astype(np.float32)
            w = cy[..., i] * cx[..., j]  # one float32 rounding of the exact product
            p[i, j] = tap * w
    r = [((p[i, 0] + p[i, 1]) + p[i, 2]) + p[i, 3] for i in range(4)]
    inner = ((r[0] + r[1]) + r[2]) + r[3]
    seq = np.zeros((H, W), np.float32)
    for i in range(4):
        for j in range(4):
            seq = seq + p[i, j]
    assert inner.dtype == np.float32 and seq.dtype == np.float32
    interior = (sx - 1 >= 0) & (sx + 2 <= W - 1) & (sy - 1 >= 0) & (sy + 2 <= H - 1)
    acc = np.where(interior, inner, seq)
    return np.clip(np.rint(acc.astype(np.float64)), 0, 65535).astype(np.uint16)


def shift_map(tx, ty):
    """The inverse map (use with inverse_map=True) that reads source (x + tx, y + ty)."""
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty]])


def rot_about_centre(rad, H, W, tx=0.0, ty=0.0, scale=1.0):
    c, s = scale * math.cos(rad), scale * math.sin(rad)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty]])


def random_u16(H, W, seed):
    return np.random.default_rng(seed).integers(0, 65536, (H, W)).astype(np.uint16)


def checkerboard(H, W, cell=2):
    """0 / 65535 in cell x cell squares.  Two-pixel squares put the taps (0, 1, 1, 0) and
    (1, 0, 0, 1) under a half-pixel shift: 38/32 and -6/32 of 65535, beyond both clamps."""
    yy, xx = np.mgrid[:H, :W]
    return ((((yy // cell) + (xx // cell)) & 1) * 65535).astype(np.uint16)


# ------------------------------------------------------------------ the weight table
def test_float32_weights_are_the_exact_rationals():
    for f in range(32):
        got, want = cubic_weights_f32(f), cubic_weights_exact(f)
        for g, w in zip(got, want):
            assert Fraction(float(g)) == w, (f, got, want)
            assert (w * 2 ** 17).denominator == 1  # an integer multiple of 2^-17
        assert sum(want) == 1


def test_quoted_weight_rows():
    assert cubic_weights_exact(0) == [0, 1, 0, 0]
    assert cubic_weights_exact(16) == [Fraction(-3, 32), Fraction(19, 32), Fraction(19, 32), Fraction(-3, 32)]
    assert cubic_weights_exact(1) == [Fraction(n, 2 ** 17) for n in (-2883, 130789, 3259, -93)]
    np.testing.assert_array_equal(CUBIC_TAB[0], np.array([0, 1, 0, 0], np.float32))
    for f in range(1, 32):  # the kernel is symmetric: the weights of 32 - f are those of f reversed
        np.testing.assert_array_equal(CUBIC_TAB[32 - f], CUBIC_TAB[f][::-1])


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("H,W", [(64, 96), (3, 5), (1, 1), (4, 4), (57, 129)])
def test_identity_returns_the_source(H, W):
    src = random_u16(H, W, H * W)
    I = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    for inv in (False, True):
        np.testing.assert_array_equal(ref_warp_affine_cubic(src, I, inv), src)


def test_integer_shift_is_a_copy_with_zeros_shifted_in():
    H, W = 40, 50
    src = random_u16(H, W, 3)
    got = ref_warp_affine_cubic(src, shift_map(3, -2), inverse_map=True)  # dst(x, y) = src(x + 3, y - 2)
    np.testing.assert_array_equal(got[2:, :W - 3], src[:H - 2, 3:])
    assert (got[:2] == 0).all() and (got[:, W - 3:] == 0).all()
    fwd = ref_warp_affine_cubic(src, shift_map(3, -2))  # forward: dst(x + 3, y - 2) = src(x, y)
    np.testing.assert_array_equal(fwd[:H - 2, 3:], src[2:, :W - 3])
    assert (fwd[H - 2:] == 0).all() and (fwd[:, :3] == 0).all()


def test_constant_65535_stays_in_the_interior():
    H, W = 32, 40
    src = np.full((H, W), 65535, np.uint16)
    M = shift_map(0.5, 0.5)
    got = ref_warp_affine_cubic(src, M, inverse_map=True)
    inner = interior_mask(M, H, W, inverse_map=True)
    assert inner.sum() == (H - 3) * (W - 3)
    assert (got[inner] == 65535).all()


def test_checkerboard_reaches_both_clamps():
    H, W = 32, 40
    src = checkerboard(H, W)
    got = ref_warp_affine_cubic(src, shift_map(0.5, 0.0), inverse_map=True)
    inner = got[4:-4, 4:-4]
    assert (inner == 0).any() and (inner == 65535).any()
    # and they are clamped values: the unclamped sums at f = 16 pass both ends of the range
    c = np.array([-3, 19, 19, -3]) / 32.0
    row = src[8].astype(np.float64)
    sums = np.array([c @ row[x - 1:x + 3] for x in range(4, W - 4)])
    assert sums.max() > 65535 + 1 and sums.min() < -1
    np.testing.assert_array_equal(np.clip(np.rint(sums), 0, 65535), got[8, 4:W - 4])


@pytest.mark.parametrize("H,W", [(3, 5), (1, 1), (3, 64), (64, 3)])
def test_small_images_never_take_the_interior_order(H, W):
    for M in (shift_map(0, 0), shift_map(0.5, 0.25), shift_map(1.0, 0.0), rot_about_centre(0.3, H, W)):
        for inv in (False, True):
            assert not interior_mask(M, H, W, inv).any()
    # and the border order is what the restatement then computes: against a scalar evaluation
    src = random_u16(H, W, 7)
    M = shift_map(0.28125, -0.40625)
    got = ref_warp_affine_cubic(src, M, inverse_map=True)
    X, Y = fixed_point_coords(M, H, W, inverse_map=True)
    for y in range(H):
        for x in range(W):
            sx, sy, fx, fy = int(X[y, x] >> 10), int(Y[y, x] >> 10), int(X[y, x] >> 5) & 31, int(Y[y, x] >> 5) & 31
            s = F32(0)
            for i in range(4):
                for j in range(4):
                    yy, xx = sy - 1 + i, sx - 1 + j
                    v = F32(src[yy, xx]) if 0 <= yy < H and 0 <= xx < W else F32(0)
                    s = s + v * (CUBIC_TAB[fy, i] * CUBIC_TAB[fx, j])
            assert got[y, x] == min(max(int(np.rint(np.float64(s))), 0), 65535)


def test_nan_map_gives_zeros():
    src = random_u16(20, 30, 1)
    M = shift_map(1.5, 0.5)
    M[1, 0] = np.nan
    for inv in (False, True):
        assert (ref_warp_affine_cubic(src, M, inv) == 0).all()


# ------------------------------------------------------------------ the accuracy claim
def _formula(x, y):
    two_pi = 2 * np.pi
    return 30000 + 12000 * np.sin(two_pi * x / 17) * np.cos(two_pi * y / 23) + 8000 * np.sin(two_pi * (x + y) / 9)


@pytest.mark.parametrize("tx,ty", [(0.5, 0.5), (0.25, 0.75)])
def test_cubic_halves_the_bilinear_resampling_error(tx, ty):
    H, W, m = 64, 96, 8
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    src = np.rint(_formula(xx, yy)).astype(np.uint16)
    truth = _formula(xx + tx, yy + ty)
    M = shift_map(tx, ty)
    cubic = ref_warp_affine_cubic(src, M, inverse_map=True).astype(np.float64)
    linear = oracle.warp_affine_u16(src, M, inverse_map=True).astype(np.float64)

    def rms(a):
        return float(np.sqrt(np.mean((a - truth)[m:-m, m:-m] ** 2)))

    print(f"shift ({tx}, {ty}): bilinear RMS {rms(linear):.1f}, cubic RMS {rms(cubic):.1f}, "
          f"ratio {rms(cubic) / rms(linear):.3f}")
    assert rms(cubic) < 0.5 * rms(linear)


# ------------------------------------------------------------------ valid_region(taps=4)
def _rigid_maps(rng, F, H, W, max_rad=0.02, max_shift=6.0):
    return np.stack([rot_about_centre(rng.uniform(-max_rad, max_rad), H, W, rng.uniform(-max_shift, max_shift),
                                      rng.uniform(-max_shift, max_shift)) for _ in range(F)])


def test_valid_region_taps4_is_the_taps2_rectangle_shrunk_by_one():
    rng = np.random.default_rng(0)
    for _ in range(20):
        H, W = int(rng.integers(40, 200)), int(rng.integers(40, 260))
        maps = _rigid_maps(rng, 5, H, W)
        y0, y1, x0, x1 = quality.valid_region(maps, H, W)
        assert quality.valid_region(maps, H, W, taps=2) == (y0, y1, x0, x1)
        assert quality.valid_region(maps, H, W, taps=4) == (y0 + 1, y1 - 1, x0 + 1, x1 - 1)
    with pytest.raises(ValueError):
        quality.valid_region(maps, H, W, taps=3)


@pytest.mark.parametrize("seed", range(6))
def test_valid_region_taps4_holds_interior_pixels_only(seed):
    rng = np.random.default_rng(100 + seed)
    H, W = int(rng.integers(48, 120)), int(rng.integers(48, 160))
    maps = _rigid_maps(rng, 6, H, W)
    y0, y1, x0, x1 = quality.valid_region(maps, H, W, taps=4)
    masks = np.stack([interior_mask(M, H, W) for M in maps])
    assert masks[:, y0:y1, x0:x1].all()
    # m = ceil(d) + 2 is a whole number of pixels, so the line just outside is still interior
    # while d lies up to a pixel below ceil(d): the next test takes the maps that attain it


@pytest.mark.parametrize("seed", range(6))
def test_valid_region_taps4_is_attained_at_whole_pixel_displacements(seed):
    """Random rigid maps whose largest displacement is a whole number of pixels on the high
    side (a translation of +d with smaller motions beside it): every pixel inside the rectangle
    is interior, and the row or column just outside is not for at least one frame."""
    rng = np.random.default_rng(200 + seed)
    H, W = int(rng.integers(48, 120)), int(rng.integers(48, 160))
    d = int(rng.integers(1, 7))
    maps = _rigid_maps(rng, 5, H, W, max_rad=0.002, max_shift=d - 0.9)
    big = shift_map(0.0, 0.0)
    big[int(rng.integers(0, 2)), 2] = -d  # forward shift by -d: the warp reads x + d (or y + d)
    maps[int(rng.integers(0, 5))] = big
    y0, y1, x0, x1 = quality.valid_region(maps, H, W, taps=4)
    assert (y0, x0) == (d + 2, d + 2)
    masks = np.stack([interior_mask(M, H, W) for M in maps])
    assert masks[:, y0:y1, x0:x1].all()
    just_out = [masks[:, y0 - 1, x0:x1], masks[:, y1, x0:x1], masks[:, y0:y1, x0 - 1], masks[:, y0:y1, x1]]
    assert any(not line.all() for line in just_out)


# ------------------------------------------------------------------ the switch without a GPU
def _va(**kw):
    return type("VA", (VideoAligner,), kw)()


def _call(va, images):
    return va.align_keypoints(images, np.zeros((0, 2)), np.zeros((0, 32), np.uint8), [], [], n_kp_global=5)


GRAY, COLOUR = np.zeros((4, 16, 16), np.uint16), np.zeros((4, 16, 16, 3), np.uint16)


@pytest.mark.parametrize("kw,images,word", [
    (dict(RANSAC_MODEL="projective"), GRAY, "projective"),
    (dict(), COLOUR, "grayscale"),
    (dict(PIECEWISE_GRID=(2, 2)), GRAY, "PIECEWISE_GRID"),
    (dict(REFINE="intensity", REFINE_GRID=(2, 2)), GRAY, "REFINE_GRID"),
])
def test_video_aligner_refuses_before_any_work(kw, images, word):
    va = _va(WARP_INTERPOLATION="cubic", **kw)
    with pytest.raises(NotImplementedError, match=word):
        _call(va, images)
    with pytest.raises(NotImplementedError, match=word):
        va.align_images(images, 5, "orb", 30)


def test_video_aligner_unknown_value():
    for bad in ("lanczos", "CUBIC", None, 3):
        with pytest.raises(ValueError, match="WARP_INTERPOLATION"):
            _call(_va(WARP_INTERPOLATION=bad), GRAY)
    assert VideoAligner.WARP_INTERPOLATION == "linear"
    assert _va(WARP_INTERPOLATION="cubic")._config(5).warp_interpolation == "cubic"
    assert VideoAligner()._config(5).warp_interpolation == "linear"


def test_config_refusals():
    cfg = pipeline.AlignConfig(n_kp_global=5)
    assert cfg.warp_interpolation == "linear" and pipeline.check_warp_interpolation(cfg, 4) == "linear"
    cubic = pipeline.AlignConfig(n_kp_global=5, warp_interpolation="cubic")
    assert pipeline.check_warp_interpolation(cubic, 3) == "cubic"
    with pytest.raises(ValueError):
        pipeline.check_warp_interpolation(pipeline.AlignConfig(n_kp_global=5, warp_interpolation="nearest"))
    with pytest.raises(NotImplementedError, match="grayscale"):
        pipeline.check_warp_interpolation(cubic, 4)
    with pytest.raises(NotImplementedError, match="projective"):
        pipeline.check_warp_interpolation(pipeline.AlignConfig(n_kp_global=5, warp_interpolation="cubic",
                                                               ransac_model="projective"))
    with pytest.raises(NotImplementedError, match="piecewise_grid"):
        pipeline.check_warp_interpolation(pipeline.AlignConfig(n_kp_global=5, warp_interpolation="cubic",
                                                               piecewise_grid=(2, 2)))


def test_stage_functions_refuse_before_touching_their_tensors():
    import torch

    fr, M = torch.zeros((2, 8, 8), dtype=torch.uint16), torch.zeros((2, 2, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="interpolation"):
        stages.warp_affine_u16(fr, M, interpolation="lanczos")
    with pytest.raises(NotImplementedError, match="grayscale"):
        stages.warp_affine_u16(torch.zeros((2, 8, 8, 3), dtype=torch.uint16), M, interpolation="cubic")
    with pytest.raises(ValueError, match="interpolation"):
        pipeline.warp_frames(fr, M, interpolation="area")
    with pytest.raises(NotImplementedError, match="3, 3"):
        pipeline.warp_frames(fr, torch.zeros((2, 3, 3), dtype=torch.float64), interpolation="cubic")
    with pytest.raises(ValueError, match="interpolation"):
        pipeline.warp_stage(fr, np.zeros((2, 2, 3)), interpolation="area")
    import inspect

    for fn in (pipeline.warp_frames, pipeline.warp_stage):  # a keyword with a default, behind the positionals
        p = inspect.signature(fn).parameters["interpolation"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "linear"


def test_custom_stage_tables_refuse_the_switch():
    import dataclasses

    from kcmc_amd import distributed as kdist

    cubic = pipeline.AlignConfig(n_kp_global=5, warp_interpolation="cubic")
    linear = pipeline.AlignConfig(n_kp_global=5)
    custom = dataclasses.replace(kdist.HIP_STAGES, warp=lambda frames, affines: frames)
    assert kdist.stages_for(linear, custom, "here") is custom
    with pytest.raises(NotImplementedError, match="custom"):
        kdist.stages_for(cubic, custom, "here")
    table = kdist.stages_for(cubic, kdist.HIP_STAGES, "here", 3)
    assert table.warp is not kdist.HIP_STAGES.warp and table.warp_params is not kdist.HIP_STAGES.warp_params
    assert table.match is kdist.HIP_STAGES.match
    with pytest.raises(NotImplementedError, match="grayscale"):
        kdist.stages_for(cubic, kdist.HIP_STAGES, "here", 4)


def test_symbol_and_null_ctx():
    assert "kcmc_warp_affine_cubic_u16" in _lib.EXPORTED_SYMBOLS
    assert "kcmc_warp_affine_cubic_u16" in _lib._SIGNATURES
    assert _lib._SIGNATURES["kcmc_warp_affine_cubic_u16"] == _lib._SIGNATURES["kcmc_warp_affine_u16"]
    L = _lib.load()
    rc = L.kcmc_warp_affine_cubic_u16(None, None, None, None, 1, 8, 8, 1, 0, None)
    assert rc == _lib.KCMC_EINVAL and b"ctx" in L.kcmc_last_error()
    with open(HEADER) as f:
        header = f.read()
    assert "kcmc_warp_affine_cubic_u16" in header and "PARITY WITH cv2 IS UNPINNED" in header
