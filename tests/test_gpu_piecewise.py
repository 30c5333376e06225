"""The piecewise-rigid mode on the device: the field warp (csrc/warp_field.hip) against the
affine warp (zero field) and against the numpy restatement of tests/test_piecewise_host.py
(random fields), the per-cell fits against oracle.ransac_rigid plus the host rules, and the
whole mode through VideoAligner.  Everything but the cell parameters (1e-9, the project's
rigid tolerance) is compared bit for bit."""
import numpy as np
import pytest
import torch

from conftest import distinct_frames
from kcmc_amd import VideoAligner, piecewise, stages
from test_gpu_multidevice import _keypoint_stack
from test_piecewise_host import (CELL_SEED, cell_stack, random_frames, ref_warp_field, restate_cells,
                                 rot_about_centre)

pytestmark = pytest.mark.gpu


def _maps(F, H, W, deg=1.0, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rot_about_centre(deg * (f + 1) / F, H, W, rng.uniform(-4, 4), rng.uniform(-4, 4))
                     for f in range(F)])


def _run(frames, M, q, dev, inverse_map=False, out=None):
    fr = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)
    return stages.warp_field_u16(fr, torch.from_numpy(np.ascontiguousarray(M)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(q, np.int32)).to(dev), out=out,
                                 inverse_map=inverse_map).cpu().numpy()


# ------------------------------------------------------------------ zero field == affine warp
@pytest.mark.parametrize("shape", [(3, 120, 264),   # partial tiles in both directions
                                   (2, 61, 75),     # odd W: element-wise staging and stores
                                   (2, 128, 512)])  # the 64-row tile rule
def test_zero_field_is_the_affine_warp(dev, shape):
    F, H, W = shape
    frames = distinct_frames(random_frames(1, H, W, seed=W)[0], F)
    fr = torch.from_numpy(frames).to(dev)
    M = _maps(F, H, W, deg=2.0, seed=H)
    M_nan = M.copy()
    M_nan[F - 1, 0, 1] = np.nan
    for grid in ((1, 1), (5, 4)):
        q = np.zeros((F,) + grid + (2,), np.int32)
        for maps in (M, M_nan):
            for inv in (False, True):
                want = stages.warp_affine_u16(fr, torch.from_numpy(maps).to(dev), inverse_map=inv).cpu().numpy()
                got = _run(fr, maps, q, dev, inverse_map=inv)
                np.testing.assert_array_equal(got, want)
        assert (got[F - 1] == 0).all() and got[0].any()  # the NaN frame is zeros


def test_zero_field_on_a_slab_that_is_not_16_byte_aligned(dev):
    F, H, W = 3, 61, 75
    whole = torch.from_numpy(distinct_frames(random_frames(1, H, W, seed=3)[0], F)).to(dev)
    slab, out = whole[1:], torch.empty_like(whole)[1:]
    assert slab.data_ptr() % 16 != 0 and out.data_ptr() % 16 != 0
    M = torch.from_numpy(_maps(2, H, W, seed=1)).to(dev)
    q = torch.zeros((2, 5, 4, 2), dtype=torch.int32, device=dev)
    want = stages.warp_affine_u16(slab.clone(), M)
    got = stages.warp_field_u16(slab, M, q, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got, want)
    # W % 8 == 0 but the slab starts 8 bytes into a 16-byte line: no 16-byte loads either
    H2, W2 = 60, 136
    flat = torch.from_numpy(random_frames(1, 2 * H2 + 1, W2, seed=9, n_sat=9)[0].reshape(-1)).to(dev)
    slab2 = flat[4:4 + 2 * H2 * W2].view(2, H2, W2)
    assert slab2.data_ptr() % 16 == 8 and slab2.is_contiguous()
    M2 = torch.from_numpy(_maps(2, H2, W2, seed=2)).to(dev)
    q2 = np.random.default_rng(0).integers(-3000, 3000, (2, 2, 3, 2)).astype(np.int32)
    got2 = stages.warp_field_u16(slab2, M2, torch.from_numpy(q2).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got2, ref_warp_field(slab2.cpu().numpy(), M2.cpu().numpy(), q2))


# ------------------------------------------------------------------ random fields == restatement
# (grid, amplitude px, shape, dark): +-40 px on (5, 4) moves neighbouring nodes of a tile by
# tens of pixels against each other, so tiles' boxes pass the 72 staged rows and gather directly
CASES = [((1, 1), 2, (3, 120, 264), False), ((2, 3), 2, (2, 61, 75), False), ((5, 4), 8, (3, 120, 264), True),
         ((16, 16), 8, (2, 128, 512), False), ((5, 4), 40, (3, 120, 264), False), ((16, 16), 2, (2, 61, 75), True),
         ((2, 3), 8, (2, 128, 512), True)]


def random_field(grid, amp, shape):
    """(q, maps) of a case of CASES."""
    F, H, W = shape
    rng = np.random.default_rng(grid[0] * 31 + amp)
    q = rng.integers(-amp * 1024, amp * 1024 + 1, (F,) + grid + (2,)).astype(np.int32)
    return q, _maps(F, H, W, deg=5.0, seed=amp)  # the last frame: 5 degrees about the centre


@pytest.mark.parametrize("grid,amp,shape,dark", CASES)
def test_random_field_is_the_restatement(dev, grid, amp, shape, dark):
    F, H, W = shape
    base = random_frames(1, H, W, seed=amp * 100 + W, hi=16384 if dark else 65536, n_sat=0 if dark else 7)[0]
    frames = distinct_frames(base, F)
    assert (frames.max() < 16384) if dark else (frames == 65535).any()
    q, M = random_field(grid, amp, shape)
    for inv in (False, True):
        np.testing.assert_array_equal(_run(frames, M, q, dev, inverse_map=inv), ref_warp_field(frames, M, q, grid, inv))


FAR_SHAPE, FAR_GRID = (2, 120, 264), (3, 3)


def far_field():
    """A field far outside the contract |q| <= 2^20, under identity maps."""
    return np.random.default_rng(1).integers(-2**31, 2**31 - 1, (FAR_SHAPE[0],) + FAR_GRID + (2,)).astype(np.int32)


def test_constant_field_is_a_shift_and_far_fields_stay_in_bounds(dev):
    F, H, W = FAR_SHAPE
    frames = distinct_frames(random_frames(1, H, W, seed=77)[0], F)
    M = np.broadcast_to(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (F, 2, 3)).copy()
    q = np.zeros((F,) + FAR_GRID + (2,), np.int32)
    q[..., 0], q[..., 1] = -3 * 1024, 2 * 1024  # source = (x - 3, y + 2)
    got = _run(frames, M, q, dev, inverse_map=True)
    np.testing.assert_array_equal(got[:, :H - 2, 3:], frames[:, 2:, :W - 3])
    assert (got[:, H - 2:] == 0).all() and (got[:, :, :3] == 0).all()
    # the contract's edge (|q| = 2^20: 1024 px, every tap outside) and far beyond it (pixels
    # unspecified, but the call must complete and stay inside its buffers)
    q[:] = 1 << 20
    assert (_run(frames, M, q, dev, inverse_map=True) == 0).all()
    guard = torch.full((F + 2, H, W), 0xABCD, dtype=torch.uint16, device=dev)
    q[:] = far_field()
    _run(frames, M, q, dev, out=guard[1:F + 1])
    g = guard.cpu().numpy()
    assert (g[0] == 0xABCD).all() and (g[F + 1] == 0xABCD).all()


# ------------------------------------------------------------------ per-cell fits
@pytest.mark.parametrize("grid", [(2, 2), (3, 4)])
def test_cell_fits_on_the_device_against_the_restatement(dev, grid):
    H, W = 200, 264
    kp_tpl, kp_ordered, lists, off = cell_stack(CELL_SEED)
    F, n_tpl = kp_ordered.shape[:2]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    pt_off, pt_idx = t(off), t(np.concatenate(lists))
    glob = stages.ransac_rigid(t(kp_ordered.reshape(-1, 2)), t(kp_tpl), pt_off, off, pt_idx=pt_idx,
                               src_frame_stride=n_tpl)
    G = glob.params.cpu().numpy()
    assert np.isfinite(G).all()
    G[4] = np.nan  # a frame without a model of its own: counted, never fitted, interpolated
    fits = piecewise.fit_cells(t(kp_ordered), t(kp_tpl), pt_off, pt_idx, off, G, H, W, grid)
    points, fitted, params, r = restate_cells(kp_tpl, kp_ordered, lists, G, H, W, grid)
    np.testing.assert_array_equal(fits.points, points)
    np.testing.assert_array_equal(fits.fitted, fitted)
    assert fits.ran.sum() >= 3 * fitted[0].size and fitted.sum() >= fits.ran.sum() // 2  # the premise: real fits
    assert not fits.fitted[4].any() and (fits.points[4] > 0).any()
    np.testing.assert_array_equal(np.isnan(fits.params), np.isnan(params))
    np.testing.assert_allclose(fits.params[fitted], params[fitted], rtol=0, atol=1e-9)
    assert np.abs(r).max() > 0.25  # the per-quadrant motion is seen
    # q: equal, except where the restatement's own r * 1024 is within 1e-4 of a half-integer
    have = ~np.isnan(G.reshape(F, 6)).any(1)
    r_all = piecewise.interpolate_fields(r, have)
    want = piecewise.quantise(r_all)
    band = np.abs(np.abs(r_all * 1024 - np.floor(r_all * 1024)) - 0.5) < 1e-4
    assert band.sum() <= 0.01 * band.size  # the seed keeps the restatement itself clear of ties
    got = piecewise.fields_from_fits(fits, G, F, 1, H, W, grid)
    np.testing.assert_array_equal(got[~band], want[~band])
    assert (np.abs(got[band].astype(np.int64) - want[band]) <= 1).all()


# ------------------------------------------------------------------ end to end
def _va(grid=None, **kw):
    return type("VA", (VideoAligner,), dict(DEVICES=[0], PIECEWISE_GRID=grid, **kw))()


def test_align_keypoints_end_to_end(dev):
    ks, frames, kq, dq = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    run = lambda va: va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40, frame_rate=100)  # noqa: E731
    off = _va()
    a0, e0, s0 = run(off)
    assert off.patch_residuals is None and off.patch_points is None and off.patch_fitted is None
    assert len(s0) >= 3
    ref = _va(QUALITY_METRICS=True)  # the grid-off run that reports its affines
    run(ref)

    va = _va((2, 2))
    a, e, s = run(va)
    F = frames.shape[0]
    assert va.patch_residuals.shape == (F, 2, 2, 2) and va.patch_residuals.dtype == np.float64
    assert va.patch_points.shape == (12, 2, 2) and va.patch_points.dtype == np.int32
    assert va.patch_fitted.shape == (12, 2, 2) and va.patch_fitted.dtype == bool
    q = np.rint(va.patch_residuals * 1024).astype(np.int32)
    np.testing.assert_array_equal(q / 1024.0, va.patch_residuals)
    np.testing.assert_array_equal(a, ref_warp_field(frames, va.affines[:F], q, (2, 2)))
    np.testing.assert_array_equal(va.affines, ref.affines)
    np.testing.assert_array_equal(e, e0)
    assert s == s0 and va.interpolated_idxs == off.interpolated_idxs
    assert va.patch_fitted.any() and (q != 0).any() and not (a == a0).all()
    assert not va.patch_fitted[s0].any()
    # the skipped frames' residuals are the interpolation of their neighbours': both sides are
    # quantised to 1/1024 px (half a step each), and a convex combination keeps that bound
    have = np.ones(F, bool)
    have[s0] = False
    interp = piecewise.interpolate_fields(np.where(have[:, None, None, None], va.patch_residuals, 0.0), have)
    assert np.abs(interp - va.patch_residuals)[s0].max() <= 1.0 / 1024 + 1e-12
    np.testing.assert_array_equal(interp[have], va.patch_residuals[have])

    one = _va((1, 1))
    a1, e1, s1 = run(one)
    np.testing.assert_array_equal(a1, a0)
    assert (one.patch_residuals == 0).all() and one.patch_residuals.shape == (F, 1, 1, 2)
    assert one.patch_fitted[[f for f in range(12) if f not in s0]].all()


def test_align_images_with_the_gpu_detector(dev):
    rng = np.random.default_rng(31)
    H, W, F = 200, 260, 9
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (F, 2))]
    shifts[F // 2] = (0, 0)
    imgs = np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts])
    va = _va((2, 3))
    a, e, s = va.align_images(imgs, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
    assert s == [] and a.shape == imgs.shape and va.patch_points.shape == (F, 2, 3)
    q = np.rint(va.patch_residuals * 1024).astype(np.int32)
    np.testing.assert_array_equal(a, ref_warp_field(imgs, va.affines[:F], q, (2, 3)))
    assert va.patch_fitted.any()
