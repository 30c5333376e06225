"""kcmc_amd.fallback on the GPU: the exact shift-search kernel (csrc/shift_search.hip)
against the numpy / Python-integer restatement of tests/test_fallback_host.py, bit for bit,
and the VideoAligner switch built on it, end to end.  Every sum is an exact integer, so every
comparison is assert_array_equal."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import test_fallback_host as host
import test_quality_host as qhost
from kcmc_amd import VideoAligner, _lib, fallback, quality
from kcmc_amd.stages import _ctx

pytestmark = pytest.mark.gpu


def _frames(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 65536, shape).astype(np.uint16)
    x.reshape(-1)[rng.integers(0, x.size, 5)] = 65535
    return x


def _raw(dev, frames_t, idx, n_sel, ref_t, rect, R):
    """The entry point itself (``idx``: a list, or None for the NULL index list)."""
    S = 2 * R + 1
    n_frames, H, W = frames_t.shape
    out = torch.full((n_sel, S, S, 5), -1, dtype=torch.int64, device=dev)  # the call zeroes it
    idx_t = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    P = ctypes.c_void_p
    _lib.check(_lib.load().kcmc_shift_search_u16(
        _ctx(dev).handle, P(frames_t.data_ptr()), n_frames, H, W, None if idx is None else P(idx_t.data_ptr()), n_sel,
        P(ref_t.data_ptr()), *rect, R, P(out.data_ptr()), P(torch.cuda.current_stream(dev).cuda_stream)))
    return out.cpu().numpy()


def _want(frames, idx, ref, rect, R):
    return host.ref_shift_search(frames, idx, ref, rect, R).astype(np.int64)


# (H, W, R, rect): 37 x 53: W % 8 != 0, the element path, odd bounds, and the rectangle at its
# limits; 64 x 96, R = 8: the 16-byte path with masked first and last vectors, 2 x 2 tiles;
# R = 12 / R = 16: two / three shifts per thread; 33 x 33: the smallest image of R = 16.
CASES = [(37, 53, 3, (5, 32, 7, 46)), (37, 53, 3, (3, 34, 3, 50)), (64, 96, 8, (8, 56, 11, 83)),
         (64, 96, 12, (12, 52, 13, 83)), (80, 120, 16, (16, 64, 17, 103)), (33, 33, 16, (16, 17, 16, 17)),
         (40, 72, 1, (1, 39, 1, 71))]


@pytest.mark.parametrize("H,W,R,rect", CASES)
def test_shift_search_equals_the_restatement(dev, H, W, R, rect):
    x = _frames((3, H, W), H * 1000 + W + R)
    ref = _frames((H, W), 77 + R)
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    assert (t.data_ptr() | ref_t.data_ptr()) % 16 == 0
    want = _want(x, [0, 1, 2], ref, rect, R)
    got = fallback.shift_search(t, [0, 1, 2], ref_t, rect, R)
    assert got.dtype == np.int64 and got.shape == (3, 2 * R + 1, 2 * R + 1, 5)
    np.testing.assert_array_equal(got, want)
    # the NULL index list: frames 0 .. n_sel - 1
    np.testing.assert_array_equal(_raw(dev, t, None, 2, ref_t, rect, R), want[:2])
    # the (0, 0) entry is kcmc_frame_stats_u16's row
    np.testing.assert_array_equal(got[:, R, R], quality.frame_stats(t, ref_t, rect))


def test_shift_search_of_a_slab_that_starts_mid_allocation(dev):
    H, W, R, rect = 64, 96, 8, (8, 56, 11, 83)
    x = _frames((3, H, W), 5)
    ref = _frames((H, W), 6)
    flat = torch.from_numpy(np.concatenate([np.zeros(4, np.uint16), x.ravel()])).to(dev)
    t = flat[4:].view(3, H, W)
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()  # W % 8 == 0, but the rows are off the 16-byte grid
    want = _want(x, [0, 1, 2], ref, rect, R)
    np.testing.assert_array_equal(fallback.shift_search(t, [0, 1, 2], ref, rect, R), want)
    # ... and a misaligned reference beside aligned frames
    rflat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), ref.ravel()])).to(dev)
    rt = rflat[1:].view(H, W)
    assert rt.data_ptr() % 16 == 2
    np.testing.assert_array_equal(_raw(dev, torch.from_numpy(x).to(dev), [0, 1, 2], 3, rt, rect, R), want)


def test_shift_search_frame_indices(dev):
    """A repeat, reversed order and indices outside the stack: all-zero rows, never read."""
    H, W, R, rect = 64, 96, 8, (8, 56, 11, 83)
    x = _frames((3, H, W), 5)
    ref = _frames((H, W), 6)
    idx = [2, 7, 0, 2, -1, 1, 3]
    want = _want(x, idx, ref, rect, R)
    assert not want[1].any() and not want[4].any() and not want[6].any() and want[0].any()
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    np.testing.assert_array_equal(_raw(dev, t, idx, len(idx), ref_t, rect, R), want)
    np.testing.assert_array_equal(fallback.shift_search(t, idx, ref_t, rect, R), want)
    # the slabs of one stack: every slab searches its own frames
    np.testing.assert_array_equal(fallback.shift_search([t[:1].clone(), t[1:].clone()], idx, ref, rect, R), want)
    assert fallback.shift_search(t, [], ref_t, rect, R).shape == (0, 17, 17, 5)


def test_shift_search_one_workgroup_walks_every_tile(dev):
    """Many selected frames: the workgroups per frame shrink to one (1536 rows), which then
    takes all four tiles of its frame in turn, and to two (768 rows)."""
    H, W, R, rect = 64, 96, 3, (3, 56, 11, 83)
    x = _frames((2, H, W), 9)
    ref = _frames((H, W), 10)
    want = _want(x, [0, 1], ref, rect, R)
    t = torch.from_numpy(x).to(dev)
    for n in (1536, 768):
        got = fallback.shift_search(t, [0, 1] * (n // 2), ref, rect, R)
        np.testing.assert_array_equal(got, np.tile(want, (n // 2, 1, 1, 1)))


def test_shift_search_saturated(dev):
    """Two all-65535 frames and reference at 1088 x 1920, R = 1, the whole interior: every
    shift gives sum(ab) = 65535^2 * n exactly, by the closed form (n = 1086 * 1918: the value is
    2^52.99, far past what 32-bit partial sums or float32 accumulation hold)."""
    H, W, R = 1088, 1920, 1
    rect = (1, H - 1, 1, W - 1)
    t = torch.from_numpy(np.full((2, H, W), 65535, np.uint16)).to(dev)
    ref = torch.from_numpy(np.full((H, W), 65535, np.uint16)).to(dev)
    v, n = 65535, (H - 2) * (W - 2)
    assert v * v * n > 2 ** 52
    want = np.empty((2, 3, 3, 5), np.int64)
    want[...] = [n * v, n * v, n * v * v, n * v * v, n * v * v]
    np.testing.assert_array_equal(fallback.shift_search(t, [0, 1], ref, rect, R), want)


def test_shift_search_validation(dev):
    H, W = 33, 40
    fr = torch.zeros((1, H, W), dtype=torch.int16, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = torch.zeros((H, W), dtype=torch.int16, device=dev)
    out = torch.zeros((17, 17, 5), dtype=torch.int64, device=dev)
    host.check_validation(_ctx(dev).handle, (fr.data_ptr(), idx.data_ptr(), ref.data_ptr(), out.data_ptr()))
    t = torch.from_numpy(_frames((2, H, W), 1)).to(dev)
    for region, radius in (((8, 26, 8, 32), 8), ((8, 25, 8, 32), 0), ((8, 25, 8, 32), 17), ((9, 9, 8, 32), 8)):
        with pytest.raises(ValueError):
            fallback.shift_search(t, [0], np.zeros((H, W), np.uint16), region, radius)
    with pytest.raises(ValueError):
        fallback.shift_search(t, [0], np.zeros((H, W + 1), np.uint16), (8, 25, 8, 32), 8)


# --------------------------------------------------------------------------- end to end
# Frames are crops of one scene: frame f shows the template's content displaced by t_f
# (frame(q) = template(q - t_f)), so its forward map is the translation -t_f.  t_f moves on a
# straight line, except that a blind frame (every descriptor one row: no match, no model) is
# off its neighbours' line by a known integer offset (dx, dy) -- the shift the fallback must
# find -- and one further blind frame by more than the radius allows.
EH, EW, EF, ER, PAD = 96, 160, 12, 8, 40
BLIND = {3: (5, -7), 5: (-7, 3), 6: (1, 0), 9: (9, -2)}  # frame: (dx, dy); 9 is over range
OVER = 9
_E2E = {}


def _line(f):
    return f - 6, -(f - 6)  # (x, y) of the straight line


def _e2e_stack():
    if not _E2E:
        rng = np.random.default_rng(17)
        scene = host.to_u16(host.blocked_scene((EH + 2 * PAD, EW + 2 * PAD), 18, sigma=800))
        template = scene[PAD:PAD + EH, PAD:PAD + EW]
        n_tpl = 60
        kp_tpl = np.stack([rng.integers(10, EW - 10, n_tpl), rng.integers(10, EH - 10, n_tpl)], 1).astype(np.float64)
        des_tpl = rng.integers(0, 256, (n_tpl, 32), dtype=np.uint8)
        frames, kq, dq, t = [], [], [], []
        for f in range(EF):
            lx, ly = _line(f)
            ox, oy = BLIND.get(f, (0, 0))
            tx, ty = lx + ox, ly + oy
            t.append((tx, ty))
            frames.append(scene[PAD - ty:PAD - ty + EH, PAD - tx:PAD - tx + EW])
            perm = rng.permutation(n_tpl)
            kq.append(kp_tpl[perm] + [tx, ty])
            dq.append(np.repeat(des_tpl[:1], n_tpl, 0) if f in BLIND else des_tpl[perm])
        _E2E.update(frames=np.ascontiguousarray(np.stack(frames)), template=template, kp_tpl=kp_tpl, des_tpl=des_tpl,
                    kq=kq, dq=dq, t=np.array(t, np.float64))
    return _E2E


def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), "FALLBACK_RADIUS": ER, **kw})()


def _run(va):
    e = _e2e_stack()
    return va.align_keypoints(e["frames"], e["kp_tpl"], e["des_tpl"], e["kq"], e["dq"], n_kp_global=40)


@pytest.fixture(scope="module")
def e2e(dev):
    """Every end-to-end run of the keypoint stack, made once."""
    out = {}
    for name, va in (("plain", VideoAligner()), ("off", _va()),
                     ("int", _va(FALLBACK="correlation", FALLBACK_SUBPIXEL=False)), ("sub", _va(FALLBACK="correlation")), ("sub2", _va((0, 0), FALLBACK="correlation")),
                     ("metrics_off", _va(QUALITY_METRICS=True)),
                     ("metrics", _va(FALLBACK="correlation", QUALITY_METRICS=True))):
        out[name] = (va, _run(va))
    return out


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert list(a[2]) == list(b[2])


def test_switch_off_changes_nothing(e2e):
    _same(e2e["off"][1], e2e["plain"][1])
    for name in ("plain", "off"):
        for attr in ("fallback_shifts", "fallback_correlations", "fallback_idxs"):
            assert getattr(e2e[name][0], attr) is None, (name, attr)
    skipped = e2e["plain"][1][2]
    assert set(skipped) >= set(BLIND)  # the premise: the blind frames have no model


def test_integer_shifts_are_the_offsets_and_the_frames_are_the_template(e2e):
    e = _e2e_stack()
    va, (aligned, eu, skipped) = e2e["int"]
    off_aligned, off_eu, off_skipped = e2e["off"][1]
    assert set(skipped) >= set(BLIND) and list(skipped) == list(off_skipped)
    assert va.interpolated_idxs == e2e["off"][0].interpolated_idxs
    print("skipped", skipped, "shifts", va.fallback_shifts, "correlations", va.fallback_correlations)
    assert va.fallback_shifts.shape == va.fallback_correlations.shape == (len(skipped), 2)
    good = [f for f in skipped if f != OVER]
    assert va.fallback_idxs == good
    y0, y1, x0, x1 = quality.valid_region(va.affines[:EF], EH, EW)
    for j, f in enumerate(skipped):
        if f == OVER:  # peak on the border: rejected, the interpolated frame stays
            assert np.isnan(va.fallback_shifts[j]).all()
            np.testing.assert_array_equal(aligned[f], off_aligned[f])
            np.testing.assert_array_equal(eu[f], off_eu[f])
            continue
        np.testing.assert_array_equal(va.fallback_shifts[j], BLIND[f])
        assert va.fallback_correlations[j, 1] == pytest.approx(1.0, abs=1e-12)  # crops of one scene
        assert va.fallback_correlations[j, 0] < 0.9
        # the sign of compose and the re-warp from the source, without an oracle
        np.testing.assert_array_equal(aligned[f, y0:y1, x0:x1], e["template"][y0:y1, x0:x1])
        np.testing.assert_allclose(va.affines[f], [[1, 0, -e["t"][f, 0]], [0, 1, -e["t"][f, 1]]], atol=1e-9)
        np.testing.assert_array_equal(eu[f, :2], va.affines[f, :, 2])
    rest = [f for f in range(EF) if f not in good]  # nothing else is touched
    np.testing.assert_array_equal(aligned[rest], off_aligned[rest])
    np.testing.assert_array_equal(eu[rest], off_eu[rest])


def test_subpixel_run_equals_the_host_restatement(e2e):
    e = _e2e_stack()
    off_va, (off_aligned, _, skipped) = e2e["off"]
    va, (aligned, eu, skipped2) = e2e["sub"]
    assert list(skipped2) == list(skipped)
    want = host.ref_fallback_pass(off_aligned, e["frames"], off_va_affines(e2e), skipped, oracle.warp_affine_u16, ER)
    w_aligned, w_affines, w_shifts, w_corr, w_idxs = want
    np.testing.assert_array_equal(va.fallback_shifts, w_shifts)
    np.testing.assert_array_equal(va.fallback_correlations, w_corr)
    assert va.fallback_idxs == w_idxs == [f for f in skipped if f != OVER]
    np.testing.assert_array_equal(va.affines[:EF], w_affines[:EF])
    np.testing.assert_array_equal(aligned, w_aligned)
    for j, f in enumerate(skipped):
        if f != OVER:
            assert (np.abs(va.fallback_shifts[j] - BLIND[f]) <= 0.5).all()
            np.testing.assert_array_equal(eu[f, :2], va.affines[f, :, 2])
    # two slabs on one GPU equal one slab
    va2, res2 = e2e["sub2"]
    _same(res2, e2e["sub"][1])
    np.testing.assert_array_equal(va2.fallback_shifts, va.fallback_shifts)
    np.testing.assert_array_equal(va2.fallback_correlations, va.fallback_correlations)
    assert va2.fallback_idxs == va.fallback_idxs
    np.testing.assert_array_equal(va2.affines, va.affines)


def off_va_affines(e2e):
    """The maps of the run without the fallback (QUALITY_METRICS publishes them)."""
    return e2e["metrics_off"][0].affines


def test_quality_metrics_measure_the_corrected_frames(e2e):
    va, (aligned, _, skipped) = e2e["metrics"]
    va0, res0 = e2e["metrics_off"]
    _same(res0, e2e["off"][1])
    _same(e2e["metrics"][1], e2e["sub"][1])
    mean0, region, corr, _ = qhost.ref_pass_metrics(aligned, va.affines, skipped)
    np.testing.assert_array_equal(va.mean_image, mean0)
    assert va.valid_region == region
    np.testing.assert_array_equal(va.frame_correlations, corr)
    print("blind frames' correlations", va0.frame_correlations[list(BLIND)], "->", va.frame_correlations[list(BLIND)])
    for f in va.fallback_idxs:
        assert va.frame_correlations[f] >= va0.frame_correlations[f]
    assert len(va.fallback_idxs) == len(BLIND) - 1


def test_switch_refusals(dev):
    e = _e2e_stack()
    args = (e["frames"], e["kp_tpl"], e["des_tpl"], e["kq"], e["dq"])
    for kw, err in ((dict(RANSAC_MODEL="projective"), NotImplementedError),
                    (dict(PIECEWISE_GRID=(2, 2)), NotImplementedError),
                    (dict(FALLBACK_RADIUS=17), ValueError), (dict(FALLBACK="phase"), ValueError)):
        with pytest.raises(err):
            _va(**{"FALLBACK": "correlation", **kw}).align_keypoints(*args, n_kp_global=40)
    rgb = np.repeat(e["frames"][..., None], 3, axis=3)
    with pytest.raises(NotImplementedError):
        _va(FALLBACK="correlation").align_keypoints(rgb, *args[1:], n_kp_global=40)
    with pytest.raises(NotImplementedError):
        _va(FALLBACK="correlation").align_images(rgb, 40, "orb", 30)


DIM = 9.6


def test_align_images_finds_a_dim_frame(dev):
    """align_images with the GPU detector and a dim frame.  A frame with fewer than two
    keypoints is an error of the matcher, as in the reference (knnMatch(k=2), VA:203), so the
    frame cannot be dimmed until it has none (1/64 of the brightness leaves a u8 range of 4,
    1/10 one keypoint): at 1/9.6 its u8 range is 26, the detector (FAST threshold 20) finds 9
    keypoints and one of them reaches the consensus -- fewer than N_KP_FRAME_SKIP, the frame
    is skipped (checked beforehand with the CPU oracle detector; the premise is asserted).
    Pearson's r ignores the gain, so the fallback finds the frame's offset from the line."""
    rng = np.random.default_rng(31)
    H, W, F, dim, off = 200, 260, 9, 2, (3, -5)
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    t = [(4, -3), (-5, 3), None, (-1, 1), (0, 0), (2, 6), (-6, -2), (5, 1), (-3, -4)]  # content displacement (x, y)
    t[dim] = ((t[1][0] + t[3][0]) // 2 + off[0], (t[1][1] + t[3][1]) // 2 + off[1])
    imgs = np.stack([scene[16 - ty:16 - ty + H, 16 - tx:16 - tx + W] for tx, ty in t])
    imgs[dim] = (imgs[dim] / DIM).astype(np.uint16)
    kw = dict(n_kp_global=60, detector_algorithm="orb", frame_rate=30)
    off_aligned, off_eu, off_skipped = _va().align_images(imgs, **kw)
    assert list(off_skipped) == [dim]  # the premise: only the dim frame has no model
    va = _va(FALLBACK="correlation", FALLBACK_SUBPIXEL=False)
    aligned, eu, skipped = va.align_images(imgs, **kw)
    print("shifts", va.fallback_shifts, "correlations", va.fallback_correlations)
    assert list(skipped) == [dim] and va.fallback_idxs == [dim]
    np.testing.assert_array_equal(va.fallback_shifts, [off])
    assert va.fallback_correlations[0, 1] > 0.99 > va.fallback_correlations[0, 0]
    y0, y1, x0, x1 = quality.valid_region(va.affines[:F], H, W)
    want = (scene[16 + y0:16 + y1, 16 + x0:16 + x1] / DIM).astype(np.uint16)  # the template's crop, dimmed
    np.testing.assert_array_equal(aligned[dim, y0:y1, x0:x1], want)
    rest = [f for f in range(F) if f != dim]
    np.testing.assert_array_equal(aligned[rest], off_aligned[rest])
    np.testing.assert_array_equal(eu[rest], off_eu[rest])
    assert tuple(eu[dim, :2]) == pytest.approx((-t[dim][0], -t[dim][1]), abs=1e-6)
