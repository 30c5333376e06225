"""kcmc_amd.refine on the GPU: the gradient-sums kernel (csrc/refine.hip) against the numpy /
Python-integer restatement of tests/test_refine_host.py, bit for bit, and the VideoAligner
switch built on it, end to end.  Every sum is an exact integer, so every kernel comparison is
assert_array_equal."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import test_fallback_host as fhost
import test_quality_host as qhost
import test_refine_host as host
from kcmc_amd import VideoAligner, _lib, refine
from kcmc_amd.stages import _ctx

pytestmark = pytest.mark.gpu


def _frames(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 65536, shape).astype(np.uint16)
    x.reshape(-1)[rng.integers(0, x.size, 5)] = 65535
    return x


def _raw(dev, frames_t, idx, n_sel, ref_t, rect, rows):
    """The entry point itself (``idx``: a list, or None for the NULL index list): [n_sel,
    n_bands, 7] int64.  The output starts as -1 everywhere: the call writes every row."""
    n_frames, H, W = frames_t.shape
    n_bands = -(-(rect[1] - rect[0]) // rows)
    out = torch.full((n_sel, n_bands, 7), -1, dtype=torch.int64, device=dev)
    idx_t = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    P = ctypes.c_void_p
    _lib.check(_lib.load().kcmc_gradient_sums_u16(
        _ctx(dev).handle, P(frames_t.data_ptr()), n_frames, H, W, None if idx is None else P(idx_t.data_ptr()), n_sel,
        P(ref_t.data_ptr()), *rect, rows, P(out.data_ptr()), P(torch.cuda.current_stream(dev).cuda_stream)))
    return out.cpu().numpy()


def _want(frames, idx, ref, rect, rows):
    return host.ref_band_sums(frames, idx, ref, rect, rows).astype(np.int64)


# (H, W, rect).  40 x 64: the 16-byte path, x0 not a multiple of 8 (masked first and last
# vectors), 8 thread columns x 32 row groups; 37 x 53: W % 8 != 0, the element path; both
# with the rectangle at its limits; 20 x 520: 64 thread columns, a wave per row segment;
# 12 x 2064: 258 vectors in 9 chunks of 32 thread columns; 7 x 2056: 256 thread columns,
# the neighbour pixels at the three wave boundaries of a row come from memory.
CASES = [(40, 64, (3, 37, 5, 59)), (40, 64, (1, 39, 1, 63)), (37, 53, (4, 33, 6, 47)), (37, 53, (1, 36, 1, 52)),
         (20, 520, (2, 18, 9, 515)), (12, 2064, (1, 11, 3, 2061)), (7, 2056, (1, 6, 8, 2055))]


@pytest.mark.parametrize("H,W,rect", CASES)
def test_gradient_sums_equal_the_restatement(dev, H, W, rect):
    x = _frames((3, H, W), H * 1000 + W)
    ref = _frames((H, W), 77 + W)
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    assert (t.data_ptr() | ref_t.data_ptr()) % 16 == 0
    h = rect[1] - rect[0]
    for rows in sorted({1, 7, h}):  # one row per band, bands that do not divide the rows, one band
        want = _want(x, [0, 1, 2], ref, rect, rows)
        got = _raw(dev, t, [0, 1, 2], 3, ref_t, rect, rows)
        assert got.shape == (3, -(-h // rows), 7)
        np.testing.assert_array_equal(got, want, err_msg=f"band_rows {rows}")
        # the NULL index list: frames 0 .. n_sel - 1
        np.testing.assert_array_equal(_raw(dev, t, None, 2, ref_t, rect, rows), want[:2])
    # the wrapper adds the bands (its own band_rows), in Python ints
    got = refine.gradient_sums(t, [0, 1, 2], ref_t, rect)
    assert got.dtype == object and got.shape == (3, 7)
    want = host.ref_gradient_sums(x, [0, 1, 2], ref, rect)
    assert [[int(v) for v in r] for r in got] == [[int(v) for v in r] for r in want]
    # sum a, sum a^2, sum a b are kcmc_frame_stats_u16's
    from kcmc_amd import quality

    st = quality.frame_stats(t, ref_t, rect)
    np.testing.assert_array_equal(got[:, :3].astype(np.int64), st[:, [0, 2, 4]])


def test_gradient_sums_of_a_slab_that_starts_mid_allocation(dev):
    H, W, rect = 40, 64, (3, 37, 5, 59)
    x = _frames((3, H, W), 5)
    ref = _frames((H, W), 6)
    flat = torch.from_numpy(np.concatenate([np.zeros(4, np.uint16), x.ravel()])).to(dev)
    t = flat[4:].view(3, H, W)
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()  # W % 8 == 0, but the rows are off the 16-byte grid
    want = host.ref_gradient_sums(x, [0, 1, 2], ref, rect)
    got = refine.gradient_sums(t, [0, 1, 2], ref, rect)
    assert [[int(v) for v in r] for r in got] == [[int(v) for v in r] for r in want]
    # ... and a misaligned reference beside aligned frames
    rflat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), ref.ravel()])).to(dev)
    rt = rflat[1:].view(H, W)
    assert rt.data_ptr() % 16 == 2
    np.testing.assert_array_equal(_raw(dev, torch.from_numpy(x).to(dev), [0, 1, 2], 3, rt, rect, 7),
                                  _want(x, [0, 1, 2], ref, rect, 7))


def test_gradient_sums_frame_indices(dev):
    """A repeat, reversed order and indices outside the stack: all-zero rows, never read."""
    H, W, rect = 40, 64, (3, 37, 5, 59)
    x = _frames((3, H, W), 5)
    ref = _frames((H, W), 6)
    idx = [2, 7, 0, 2, -1, 1, 3]
    want = _want(x, idx, ref, rect, 7)
    assert not want[1].any() and not want[4].any() and not want[6].any() and want[0].any()
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    np.testing.assert_array_equal(_raw(dev, t, idx, len(idx), ref_t, rect, 7), want)
    whole = host.ref_gradient_sums(x, idx, ref, rect)
    got = refine.gradient_sums(t, idx, ref_t, rect)
    assert [[int(v) for v in r] for r in got] == [[int(v) for v in r] for r in whole]
    # the slabs of one stack: every slab sums its own frames
    got = refine.gradient_sums([t[:1].clone(), t[1:].clone()], idx, ref, rect)
    assert [[int(v) for v in r] for r in got] == [[int(v) for v in r] for r in whole]
    # n_sel = 0
    assert refine.gradient_sums(t, [], ref_t, rect).shape == (0, 7)
    assert _raw(dev, t, [], 0, ref_t, rect, 7).shape == (0, 5, 7)


@pytest.mark.parametrize("pattern", ["columns", "rows"])
def test_gradient_sums_saturated(dev, pattern):
    """All-65535 frames at 258 x 4098 against a reference of period 4 (0, 0, 65535, 65535) along
    the columns resp. the rows: every gradient is +-65535 or 0, the weights reach +-2048.
    band_rows = 255 is the largest the bound allows (255 * 4096 * 4096 < 2^32) and equals the
    Python-int sums; 256 * 4096 * 4096 = 2^32 is refused."""
    H, W = 258, 4098
    rect = (1, H - 1, 1, W - 1)
    line = np.array([0, 0, 65535, 65535], np.uint16)
    ref = np.tile(line, (H, W // 4 + 1))[:, :W] if pattern == "columns" else np.tile(line[:, None], (H // 4 + 1, W))[:H]
    ref = np.ascontiguousarray(ref)
    x = np.full((2, H, W), 65535, np.uint16)
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    want = _want(x, [0, 1], ref, rect, 255)
    assert want[:, 0, 1:3].min() > 2 ** 50  # sum a^2, sum a b: far past 32-bit or float32 partial sums
    np.testing.assert_array_equal(_raw(dev, t, [0, 1], 2, ref_t, rect, 255), want)
    with pytest.raises(ValueError, match="2\\^32"):
        _raw(dev, t, [0, 1], 2, ref_t, rect, 256)


def test_gradient_sums_validation(dev):
    H, W = 33, 40
    fr = torch.zeros((1, H, W), dtype=torch.int16, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = torch.zeros((H, W), dtype=torch.int16, device=dev)
    out = torch.zeros((4, 7), dtype=torch.int64, device=dev)
    host.check_validation(_ctx(dev).handle, (fr.data_ptr(), idx.data_ptr(), ref.data_ptr(), out.data_ptr()))
    t = torch.from_numpy(_frames((2, H, W), 1)).to(dev)
    for region in ((0, 32, 1, 39), (1, 33, 1, 39), (1, 32, 1, 40), (9, 9, 8, 32)):
        with pytest.raises(ValueError):
            refine.gradient_sums(t, [0], np.zeros((H, W), np.uint16), region)
    with pytest.raises(ValueError):
        refine.gradient_sums(t, [0], np.zeros((H, W + 1), np.uint16), (1, 32, 1, 39))
    with pytest.raises(ValueError):
        refine.gradient_sums(t, [0], np.zeros((H, W), np.uint16), (1, 32, 1, 39), rows=0)


# --------------------------------------------------------------------------- end to end
# Frames are integer crops of one sampling of the analytic texture of test_refine_host: frame
# f shows the template's content displaced by t_f, so its true forward map is the translation
# -t_f.  Every frame's keypoints carry a common offset of 0.3 - 0.5 px in a random direction --
# the jitter a map fitted to a few keypoints has -- which RANSAC reproduces exactly; the
# refinement has to take it out again.  In the second stack one frame is blind (every
# descriptor one row: no match, no model) and off its neighbours' line by an integer offset,
# which the correlation fallback finds before the refinement runs.
EH, EW, EF, PAD = 96, 128, 12, 12
BLIND, BLIND_OFF = 5, (3, -2)
_E2E = {}


def _e2e_stack(blind=False):
    if blind not in _E2E:
        rng = np.random.default_rng(29)
        tex = host.Texture(11)
        scene = fhost.to_u16(np.rint(tex(*host.grid(EH + 2 * PAD, EW + 2 * PAD))))
        scene = fhost.to_u16(scene + rng.normal(0, 40, scene.shape))
        template = scene[PAD:PAD + EH, PAD:PAD + EW]
        n_tpl = 60
        kp_tpl = np.stack([rng.integers(10, EW - 10, n_tpl), rng.integers(10, EH - 10, n_tpl)], 1).astype(np.float64)
        des_tpl = rng.integers(0, 256, (n_tpl, 32), dtype=np.uint8)
        ang = rng.uniform(0, 2 * np.pi, EF)
        jit = rng.uniform(0.3, 0.5, EF)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        t = rng.integers(-3, 4, (EF, 2))
        if blind:
            t[BLIND] = (t[BLIND - 1] + t[BLIND + 1]) // 2 + BLIND_OFF
        frames, kq, dq = [], [], []
        for f in range(EF):
            tx, ty = (int(v) for v in t[f])
            frames.append(scene[PAD - ty:PAD - ty + EH, PAD - tx:PAD - tx + EW])
            perm = rng.permutation(n_tpl)
            kq.append(kp_tpl[perm] + [tx, ty] + jit[f])
            dq.append(np.repeat(des_tpl[:1], n_tpl, 0) if blind and f == BLIND else des_tpl[perm])
        truth = np.array([[[1, 0, -tx], [0, 1, -ty]] for tx, ty in t], np.float64)
        _E2E[blind] = dict(frames=np.ascontiguousarray(np.stack(frames)), template=template, kp_tpl=kp_tpl,
                           des_tpl=des_tpl, kq=kq, dq=dq, truth=truth)
    return _E2E[blind]


def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), **kw})()


def _run(va, blind=False):
    e = _e2e_stack(blind)
    return va.align_keypoints(e["frames"], e["kp_tpl"], e["des_tpl"], e["kq"], e["dq"], n_kp_global=40)


@pytest.fixture(scope="module")
def e2e(dev):
    """Every end-to-end run, made once."""
    out = {}
    on = dict(REFINE="intensity")
    for name, va, blind in (("plain", VideoAligner(), False), ("off", _va(), False), ("on", _va(**on), False),
                            ("on2", _va((0, 0), **on), False),
                            ("translation", _va(REFINE_MOTION="translation", REFINE_ITERS=1, **on), False),
                            ("metrics_off", _va(QUALITY_METRICS=True), False),
                            ("metrics", _va(QUALITY_METRICS=True, **on), False),
                            ("b_off", _va(QUALITY_METRICS=True), True),
                            ("b_refine", _va(**on), True),
                            ("b_fallback", _va(FALLBACK="correlation", QUALITY_METRICS=True), True),
                            ("b_both", _va(FALLBACK="correlation", **on), True)):
        out[name] = (va, _run(va, blind))
    return out


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert list(a[2]) == list(b[2])


def _check_against_restatement(va, result, sources, before_aligned, before_affines, skipped, **kw):
    """The run's maps, steps and correlations equal the host restatement run on the frames
    and maps of the run without the refinement, within the solver tolerance."""
    aligned, eu, skipped2 = result
    assert list(skipped2) == list(skipped)
    w_aligned, w_affines, w_steps, w_corr, w_idxs = host.ref_refine_pass(
        before_aligned, sources, before_affines, skipped, oracle.warp_affine_u16, **kw)
    n = len(sources)
    assert va.refine_steps.shape == w_steps.shape and va.refine_correlations.shape == w_corr.shape
    np.testing.assert_allclose(va.refine_steps, w_steps, rtol=0, atol=host.SOLVER_TOL)
    np.testing.assert_allclose(va.refine_correlations, w_corr, rtol=0, atol=host.SOLVER_TOL)
    np.testing.assert_allclose(va.affines[:n], w_affines[:n], rtol=0, atol=host.SOLVER_TOL)
    assert va.refine_idxs == w_idxs
    for f in range(n):  # every frame is the warp of its source with its map
        np.testing.assert_array_equal(aligned[f], oracle.warp_affine_u16(sources[f], va.affines[f]), err_msg=str(f))
    for f in va.refine_idxs:
        np.testing.assert_array_equal(eu[f, :2], va.affines[f, :, 2])
    return w_idxs


def test_switch_off_changes_nothing(e2e):
    _same(e2e["off"][1], e2e["plain"][1])
    for name in ("plain", "off"):
        for attr in ("refine_steps", "refine_correlations", "refine_idxs"):
            assert getattr(e2e[name][0], attr) is None, (name, attr)
    assert list(e2e["plain"][1][2]) == []  # the premise: every frame has a model


def test_refined_run_equals_the_host_restatement_and_lowers_the_error(e2e):
    e = _e2e_stack()
    off_aligned, off_eu, skipped = e2e["off"][1]
    off_affines = e2e["metrics_off"][0].affines
    va, res = e2e["on"]
    idxs = _check_against_restatement(va, res, e["frames"], off_aligned, off_affines, skipped, iters=2)
    assert va.refine_steps.shape == (EF, 2, 3) and va.refine_correlations.shape == (EF, 3)
    before, after = host.rms_error(off_affines[:EF], e["truth"]), host.rms_error(va.affines[:EF], e["truth"])
    print("RMS translation error", before, "->", after, "stepped", idxs)
    print("steps", va.refine_steps[:, :, :2].round(3).tolist())
    assert 0.3 <= before <= 0.5  # the premise: RANSAC reproduces the jitter
    assert after < before
    assert len(idxs) > 0
    c = va.refine_correlations
    assert (c[:, 2] >= c[:, 1]).all()  # columns 1 and 2 share the last iteration's reference image
    assert va.interpolated_idxs == e2e["off"][0].interpolated_idxs
    rest = [f for f in range(EF) if f not in idxs]
    np.testing.assert_array_equal(res[0][rest], off_aligned[rest])
    np.testing.assert_array_equal(res[1][rest], off_eu[rest])
    # two slabs on one GPU equal one slab
    va2, res2 = e2e["on2"]
    _same(res2, res)
    np.testing.assert_array_equal(va2.refine_steps, va.refine_steps)
    np.testing.assert_array_equal(va2.refine_correlations, va.refine_correlations)
    assert va2.refine_idxs == va.refine_idxs
    np.testing.assert_array_equal(va2.affines, va.affines)


def test_translation_motion_leaves_the_rotation_alone(e2e):
    e = _e2e_stack()
    off_aligned, _, skipped = e2e["off"][1]
    off_affines = e2e["metrics_off"][0].affines
    va, res = e2e["translation"]
    _check_against_restatement(va, res, e["frames"], off_aligned, off_affines, skipped, iters=1, motion="translation")
    assert va.refine_steps.shape == (EF, 1, 3) and not va.refine_steps[:, :, 2].any()
    np.testing.assert_array_equal(va.affines[:EF, :, :2], off_affines[:EF, :, :2])
    assert host.rms_error(va.affines[:EF], e["truth"]) < host.rms_error(off_affines[:EF], e["truth"])


def test_quality_metrics_measure_the_refined_frames(e2e):
    va, (aligned, _, skipped) = e2e["metrics"]
    va0, res0 = e2e["metrics_off"]
    _same(res0, e2e["off"][1])
    _same(e2e["metrics"][1], e2e["on"][1])
    mean0, region, corr, _ = qhost.ref_pass_metrics(aligned, va.affines, skipped)
    np.testing.assert_array_equal(va.mean_image, mean0)
    assert va.valid_region == region
    np.testing.assert_array_equal(va.frame_correlations, corr)
    print("mean correlation", va0.frame_correlations.mean(), "->", va.frame_correlations.mean())
    assert va.frame_correlations.mean() > va0.frame_correlations.mean()
    np.testing.assert_array_equal(va.refine_steps, e2e["on"][0].refine_steps)


def test_the_fallback_runs_before_the_refinement(e2e):
    e = _e2e_stack(blind=True)
    va0, (a0, _, skipped) = e2e["b_off"]
    assert list(skipped) == [BLIND]  # the premise: only the blind frame has no model
    vaf, (af, _, _) = e2e["b_fallback"]
    assert vaf.fallback_idxs == [BLIND]
    va, res = e2e["b_both"]
    assert va.fallback_idxs == [BLIND]
    np.testing.assert_array_equal(va.fallback_shifts, vaf.fallback_shifts)
    # the refinement starts from the fallback's frames and maps ...
    _check_against_restatement(va, res, e["frames"], af, vaf.affines, skipped, iters=2)
    # ... so the blind frame enters it registered; without the fallback it enters with its interpolated map
    vr, resr = e2e["b_refine"]
    assert vr.fallback_idxs is None
    _check_against_restatement(vr, resr, e["frames"], a0, va0.affines, skipped, iters=2)
    print("blind frame's r before the refinement: interpolated", vr.refine_correlations[BLIND, 0], "after the fallback",
          va.refine_correlations[BLIND, 0])
    assert va.refine_correlations[BLIND, 0] > vr.refine_correlations[BLIND, 0]
    assert list(res[2]) == [BLIND] and va.interpolated_idxs == va0.interpolated_idxs
    print("blind frame's map error", va.affines[BLIND, :, 2] - e["truth"][BLIND, :, 2])
