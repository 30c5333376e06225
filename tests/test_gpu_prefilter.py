"""kcmc_amd.prefilter on the GPU: the band-pass kernel (csrc/band_filter.hip) against the numpy
restatement of tests/test_prefilter_host.py, bit for bit -- frames smaller than the window, every
clipped window size, the strip and chunk seams of every radius, the divide's upper bound, views
off the 16-byte grid, guard elements, slabs, a seeded sweep, a stack beyond 2^31 elements -- and the
switch end to end through VideoAligner and pipeline.align_frames."""
import numpy as np
import pytest
import torch

from kcmc_amd import VideoAligner, _intensity, _lib, pipeline, prefilter, quality, stages
from test_bidi_host import ref_shift_rows
from test_gpu_bidi import SENTINEL, _scene_stack, assert_same_run, guarded, guards_intact
from test_prefilter_host import RADII, check_validation, random_u16, ref_box_bandpass

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------ the kernel, bit for bit
# (1, 1); (3, 50), (40, 7): the window wider than the frame along one axis; (33, 33); (70, 70), (67, 131)
# with r = 32: every clipped row / column count from 33 to 65, odd W, two row chunks
SHAPES = [(1, 1), (3, 50), (40, 7), (33, 33), (70, 70), (67, 131)]


def seam_shapes(s, r):
    """One strip and one row chunk plus a pixel each way; exactly two strips and two chunks.  The
    strip width and the cut into chunks are asked of the library (six frames, as content() makes)."""
    tw = prefilter.launch_plan(6, 1, 1, s, r)[0]
    shapes = [(65, tw + 1), (64, 2 * tw)]
    assert prefilter.launch_plan(6, *shapes[0], s, r) == (tw, 2, 2, 33)
    assert prefilter.launch_plan(6, *shapes[1], s, r) == (tw, 2, 2, 32)
    return shapes


def content(H, W, seed):
    """Six frames: random full range twice, all 65535 (the divide's bound at every n), all 0, 65535
    with a single 0 and the reverse (rounding at the half)."""
    x = random_u16((6, H, W), seed)
    x[2], x[3], x[4], x[5] = 65535, 0, 65535, 0
    x[4, H // 2, W // 3] = 0
    x[5, H // 3, W // 2] = 65535
    return x


@pytest.mark.parametrize("s,r", RADII)
def test_kernel_is_the_restatement(dev, s, r):
    for H, W in SHAPES + seam_shapes(s, r):
        x = content(H, W, 7 * H + W)
        t = torch.from_numpy(x).to(dev)
        got = prefilter.box_bandpass(t, s, r)
        assert got.data_ptr() != t.data_ptr() and got.dtype == torch.uint16 and got.shape == t.shape
        np.testing.assert_array_equal(got.cpu().numpy(), ref_box_bandpass(x, s, r), err_msg=f"{H} x {W}")
        np.testing.assert_array_equal(t.cpu().numpy(), x)


def test_single_pixels_at_the_half(dev):
    """A lone dark pixel in a bright frame and the reverse, at every position class of a frame with
    every clipped window size: the sums sit next to multiples of n."""
    H, W = 67, 70
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (33, 35), (1, 34), (40, 2)]
    x = np.zeros((2 * len(spots), H, W), np.uint16)
    x[::2] = 65535
    for k, (y, xx) in enumerate(spots):
        x[2 * k, y, xx] = 0
        x[2 * k + 1, y, xx] = 65535
    t = torch.from_numpy(x).to(dev)
    for s, r in ((0, 32), (4, 32), (4, 0), (1, 2), (3, 17)):
        np.testing.assert_array_equal(prefilter.box_bandpass(t, s, r).cpu().numpy(), ref_box_bandpass(x, s, r))


def test_more_jobs_than_workgroups_and_whole_frame_columns(dev):
    """2^20 + 5 frames of one pixel: the workgroups stride over the jobs; 2100 frames of 70 x 9: enough
    strips that a frame of more than two chunk heights is walked whole."""
    x = random_u16(((1 << 20) + 5, 1, 1), 1)
    t = torch.from_numpy(x).to(dev)
    np.testing.assert_array_equal(prefilter.box_bandpass(t, 1, 0).cpu().numpy(), x)
    assert not prefilter.box_bandpass(t, 0, 1).cpu().numpy().any()
    x = random_u16((2100, 70, 9), 2)
    np.testing.assert_array_equal(prefilter.box_bandpass(torch.from_numpy(x).to(dev), 2, 12).cpu().numpy(),
                                  ref_box_bandpass(x, 2, 12))


@pytest.mark.parametrize("H,W,s,r", [(1121, 40, 1, 0), (2160, 40, 1, 12), (2050, 24, 1, 12), (2160, 300, 4, 32)])
def test_one_tall_frame_in_many_chunks(dev, H, W, s, r):
    """A single frame -- what a masked_template or a refined template is -- of a height at which
    ceil(H / (H // 32)) chunks would overshoot the frame: the plan has no empty chunk, the source
    view ends where its buffer ends, and the guard elements around the output stay intact."""
    tw, strips, chunks, rows = prefilter.launch_plan(1, H, W, s, r)
    assert chunks > 32 and (chunks - 1) * rows < H <= chunks * rows
    x = random_u16((1, H, W), H + W)
    buf = torch.from_numpy(np.concatenate([np.zeros(3, np.uint16), x.reshape(-1)])).to(dev)
    src = buf[3:].view(1, H, W)  # the last pixel is the buffer's last element
    dbuf, dst = guarded(dev, np.full_like(x, SENTINEL), 1)
    got = prefilter.box_bandpass(src, s, r, out=dst)
    np.testing.assert_array_equal(got.cpu().numpy(), ref_box_bandpass(x, s, r))
    assert guards_intact(dbuf, x, 1)


def test_frame_offsets_beyond_2_to_the_31(dev):
    """8200 frames of 512 x 512 are 2.15e9 elements: the last frames sit beyond a 32-bit offset."""
    F, H, W = 8200, 512, 512
    base = random_u16((8, H, W), 3)
    src = torch.empty((F, H, W), dtype=torch.uint16, device=dev)
    bits = src.view(torch.int16)  # the same bits, in a dtype every tensor operation supports
    bits.view(F // 8, 8, H, W).copy_(torch.from_numpy(base.view(np.int16)).to(dev))
    bits[F - 1, 5, 7] = 12345
    got = prefilter.box_bandpass(src, 1, 12)
    want = ref_box_bandpass(base, 1, 12)
    np.testing.assert_array_equal(got[:8].cpu().numpy(), want)
    np.testing.assert_array_equal(got[F - 9:F - 1].cpu().numpy(), want[[7, 0, 1, 2, 3, 4, 5, 6]])
    last = base[7].copy()
    last[5, 7] = 12345
    np.testing.assert_array_equal(got[F - 1].cpu().numpy(), ref_box_bandpass(last, 1, 12))
    del src, got, bits
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------ views and slabs
@pytest.mark.parametrize("H,W", [(6, 24), (5, 13), (64, 136)])
def test_views_one_element_into_their_buffers(dev, H, W):
    """Source and output start one element into their allocations (off the 16-byte grid), each alone
    and both; the guard frames around the output stay intact."""
    x = random_u16((3, H, W), H + W)
    for so, do in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for s, r in ((1, 12), (4, 32), (2, 0)):
            sbuf, src = guarded(dev, x, so)
            dbuf, dst = guarded(dev, np.full_like(x, SENTINEL), do)
            assert src.data_ptr() % 16 == (2 * (so + H * W)) % 16
            got = prefilter.box_bandpass(src, s, r, out=dst)
            assert got.data_ptr() == dst.data_ptr()
            np.testing.assert_array_equal(got.cpu().numpy(), ref_box_bandpass(x, s, r), err_msg=f"{so} {do} {s} {r}")
            np.testing.assert_array_equal(src.cpu().numpy(), x)
            assert guards_intact(dbuf, x, do) and guards_intact(sbuf, x, so)


def test_slabs_arguments_and_overlap(dev):
    H, W = 33, 41
    x = random_u16((5, H, W), 9)
    t = torch.from_numpy(x).to(dev)
    want = ref_box_bandpass(x, 1, 12)
    slabs = [t[:2], t[2:]]  # views of one allocation, the second off the 16-byte grid
    assert slabs[0].data_ptr() % 16 == 0 and slabs[1].data_ptr() % 16 == 4 and slabs[1].is_contiguous()
    got = prefilter.box_bandpass(slabs, 1, 12)  # out=None: new tensors
    assert isinstance(got, list) and [g.shape[0] for g in got] == [2, 3]
    np.testing.assert_array_equal(torch.cat(got).cpu().numpy(), want)
    np.testing.assert_array_equal(t.cpu().numpy(), x)
    o = torch.zeros_like(t)
    outs = [o[:2], o[2:]]  # out given, likewise views
    same = prefilter.box_bandpass(slabs, 1, 12, out=outs)
    assert [a.data_ptr() for a in same] == [a.data_ptr() for a in outs]
    np.testing.assert_array_equal(o.cpu().numpy(), want)
    # overlap is refused and nothing is written: the input itself, a partial overlap either way round,
    # the other slab of the same stack
    flat = torch.zeros(2 * x.size, dtype=torch.uint16, device=dev)
    a = flat[:x.size].view(x.shape)
    a.copy_(t)
    with pytest.raises(ValueError, match="overlap"):
        prefilter.box_bandpass(a, 1, 12, out=a)
    for off in (1, W, H * W, x.size - 1):
        b = flat[off:off + x.size].view(x.shape)
        with pytest.raises(ValueError, match="overlap"):
            prefilter.box_bandpass(a, 1, 12, out=b)
        with pytest.raises(ValueError, match="overlap"):
            prefilter.box_bandpass(b, 1, 12, out=a)
    with pytest.raises(ValueError, match="overlap"):
        prefilter.box_bandpass(slabs, 1, 12, out=[torch.empty_like(slabs[0]), t[:3]])
    np.testing.assert_array_equal(a.cpu().numpy(), x)
    for bad in ((0, 0), (5, 9), (2, 2), (1, 33), (True, 3), (1.0, 3)):
        with pytest.raises(ValueError):
            prefilter.box_bandpass(t, *bad)
    with pytest.raises(ValueError):
        prefilter.box_bandpass(t, 1, 12, out=o[:4])  # shape
    with pytest.raises(ValueError):
        prefilter.box_bandpass(slabs, 1, 12, out=[o])  # one tensor per slab
    with pytest.raises(TypeError):
        prefilter.box_bandpass(t.to(torch.int16), 1, 12)
    with pytest.raises(TypeError):
        prefilter.box_bandpass(t, 1, 12, out=o.to(torch.int16))
    with pytest.raises(ValueError):
        prefilter.box_bandpass(t[0], 1, 12)  # not 3-D
    empty = prefilter.box_bandpass(t[:0], 1, 12)
    assert empty.shape == (0, H, W) and empty.dtype == torch.uint16
    assert [e.shape[0] for e in prefilter.box_bandpass([t[:0], t], 4, 32)] == [0, 5]


def test_entry_point_validates_with_device_pointers(dev):
    src = torch.zeros((2, 33, 40), dtype=torch.uint16, device=dev)
    dst = torch.zeros((2, 33, 40), dtype=torch.uint16, device=dev)
    check_validation(_lib.context(0).handle, (src.data_ptr(), dst.data_ptr()))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- a seeded sweep
def sweep_case(seed):
    import sweep_cases

    rng = np.random.default_rng([20240, seed])
    s = int(rng.integers(0, 5))
    r = 0 if (s > 0 and rng.random() < 0.25) else int(rng.integers(s + 1, 33))
    if rng.random() < 0.3:  # heights at the chunk seams (a strip is wider than any W here)
        H = int(rng.choice([1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160]))
        W = int(rng.choice([1, 2, 159, 160]))
    else:
        H, W = int(rng.integers(1, 161)), sweep_cases._width(rng, 1, 160)
    F = int(rng.integers(1, 4))
    return dict(s=s, r=r, x=sweep_cases._values(rng, (F, H, W)), so=int(rng.choice([0, 1, 3, 8])),
                do=int(rng.choice([0, 1, 5, 8])))


def test_seeded_sweep(dev):
    for seed in range(160):
        c = sweep_case(seed)
        x, s, r = c["x"], c["s"], c["r"]
        sbuf, src = guarded(dev, x, c["so"])
        dbuf, dst = guarded(dev, np.full_like(x, SENTINEL), c["do"])
        got = prefilter.box_bandpass(src, s, r, out=dst).cpu().numpy()
        what = f"seed {seed}: {x.shape}, radii ({s}, {r}), offsets {c['so']} {c['do']}"
        np.testing.assert_array_equal(got, ref_box_bandpass(x, s, r), err_msg=what)
        assert guards_intact(dbuf, x, c["do"]) and guards_intact(sbuf, x, c["so"]), what


# ------------------------------------------------------------------------------ end to end
S, R = 1, 12


def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), **kw})()


def _on(devices=(0,), **kw):
    return _va(devices, DETECT_SMOOTH_RADIUS=S, DETECT_BACKGROUND_RADIUS=R, **kw)


def _run(va, x, **kw):
    aligned, eu, skipped = va.align_images(x, n_kp_global=60, detector_algorithm="orb", frame_rate=30, **kw)
    aligned = aligned.cpu().numpy() if isinstance(aligned, torch.Tensor) else aligned
    return dict(aligned=aligned, eu=eu, skipped=list(skipped), affines=va.affines,
                interpolated=list(va.interpolated_idxs))


def _warped(dev, raw, affines):
    maps = torch.from_numpy(np.ascontiguousarray(affines[:len(raw)], np.float64)).to(dev)
    return stages.warp_affine_u16(torch.from_numpy(raw).to(dev), maps).cpu().numpy()


@pytest.fixture(scope="module")
def scene(dev):
    """The 9-frame 200 x 260 scene stack of tests/test_gpu_bidi.py, its filtered copy, the plain
    aligner's run on the copy and the raw stack warped by that run's maps."""
    raw = _scene_stack()
    filt = ref_box_bandpass(raw, S, R)
    plain = _run(_va(), filt)
    assert np.isfinite(plain["eu"]).all() and len(plain["skipped"]) < len(raw) // 2
    want = dict(plain, aligned=_warped(dev, raw, plain["affines"]))
    assert (want["aligned"] != plain["aligned"]).any()
    return dict(raw=raw, filt=filt, want=want)


@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one slab", "two slabs"])
def test_switch_detects_on_the_filtered_stack_and_warps_the_raw_one(dev, scene, devices):
    raw, want = scene["raw"], scene["want"]
    va = _on(devices)
    assert_same_run(_run(va, raw), want, "host input")
    assert va.prefilter_radii == (S, R)
    assert va.prefilter_brightest_px == np.percentile(scene["filt"], 99.99)
    t = torch.from_numpy(raw).to(dev)
    assert_same_run(_run(_on(devices), t), want, "device input")
    np.testing.assert_array_equal(t.cpu().numpy(), raw)  # the caller's tensor is never written
    # a masked_template equal to the raw template frame is filtered like the stack's own frame
    assert_same_run(_run(_on(devices), raw, masked_template=raw[int(len(raw) * 0.5)]), want, "masked template")
    va.DETECT_SMOOTH_RADIUS = va.DETECT_BACKGROUND_RADIUS = 0  # off again: the results are reset
    _run(va, raw)
    assert va.prefilter_radii is None and va.prefilter_brightest_px is None


def test_switch_follows_the_phase_correction(dev, scene):
    raw = scene["raw"]
    assert_same_run(_run(_on(BIDI_PHASE=3), raw), _run(_on(), ref_shift_rows(raw, 3)))


def test_a_flattened_stack_is_an_alignment_error(dev):
    flat = np.full((4, 40, 50), 3000, np.uint16)
    va = _on()
    with pytest.raises(VideoAligner.AlignmentError, match="DETECT_SMOOTH_RADIUS = 1, DETECT_BACKGROUND_RADIUS = 12"):
        va.align_images(flat, 60, "orb", 30)
    assert va.prefilter_brightest_px == 0
    with pytest.raises(VideoAligner.AlignmentError, match="smoothing radius 1, background radius 12"):
        pipeline.align_frames(torch.from_numpy(flat).to(dev), pipeline.AlignConfig(n_kp_global=60), prefilter=(S, R))


class _RecordingDetector:
    """A host detector (not the GPU detector's class, so align_images takes the host path) that
    keeps the images it is handed and answers with the GPU detector's keypoints."""
    seen = []

    def __init__(self):
        from kcmc_amd.video_aligner import GpuOrbDetector

        self.inner = GpuOrbDetector()

    def detectAndCompute(self, image, mask=None):  # noqa: N802
        type(self).seen.append(np.array(image))
        return self.inner.detectAndCompute(image, mask)


def test_a_host_detector_is_handed_the_scaled_filtered_frames(dev, scene):
    raw, filt = scene["raw"], scene["filt"]
    _RecordingDetector.seen = []
    det = dict(VideoAligner.DETECTOR_CONSTRUCTOR_DICT, recording=_RecordingDetector)
    va = _on(DETECTOR_CONSTRUCTOR_DICT=det)
    aligned, eu, skipped = va.align_images(raw, n_kp_global=60, detector_algorithm="recording", frame_rate=30)
    u8 = stages.max_scale_lut(np.percentile(filt, 99.99))[filt]
    seen = _RecordingDetector.seen
    assert len(seen) == 1 + len(raw)
    np.testing.assert_array_equal(seen[0], u8[int(len(raw) * 0.5)])  # the template first
    np.testing.assert_array_equal(np.stack(seen[1:]), u8)
    assert np.isfinite(eu).all()
    np.testing.assert_array_equal(aligned, _warped(dev, raw, va.affines))


@pytest.mark.parametrize("algorithm", ["orb", "recording"])
def test_template_refinement_filters_the_refined_template_only_for_detection(dev, scene, algorithm):
    """TEMPLATE_REFINE_ITERS = 1: template_image is the mean of the selected raw aligned frames of
    the first pass (not filtered), and the detector sees its filtered, max-scaled copy."""
    raw, filt = scene["raw"], scene["filt"]
    det = dict(VideoAligner.DETECTOR_CONSTRUCTOR_DICT, recording=_RecordingDetector)
    first = _on(DETECTOR_CONSTRUCTOR_DICT=det, QUALITY_METRICS=True)
    a1, _, skipped1 = first.align_images(raw, 60, algorithm, 30)
    sel0 = np.flatnonzero(_intensity.sample_mask(len(raw), 1, skipped1)).tolist()
    best = quality.select_top(first.frame_correlations, sel0, 0.5)
    n = len(best)
    mean = ((a1[best].astype(np.int64).sum(0) + n // 2) // n).astype(np.uint16)
    _RecordingDetector.seen = []
    va = _on(DETECTOR_CONSTRUCTOR_DICT=det, TEMPLATE_REFINE_ITERS=1)
    aligned, eu, skipped = va.align_images(raw, 60, algorithm, 30)
    np.testing.assert_array_equal(va.template_image, mean)
    assert np.isfinite(eu).all() and len(va.correlation_history) == 2
    np.testing.assert_array_equal(aligned, _warped(dev, raw, va.affines))
    if algorithm == "recording":
        u8 = stages.max_scale_lut(np.percentile(filt, 99.99))[ref_box_bandpass(mean, S, R)]
        np.testing.assert_array_equal(_RecordingDetector.seen[-1], u8)


def test_align_frames_takes_the_prefilter(dev, scene):
    raw, filt = scene["raw"], scene["filt"]
    cfg = pipeline.AlignConfig(n_kp_global=60)
    plain = pipeline.align_frames(torch.from_numpy(filt).to(dev), cfg)
    t = torch.from_numpy(raw).to(dev)
    got = pipeline.align_frames(t, cfg, prefilter=(S, R))
    np.testing.assert_array_equal(got.affines, plain.affines)
    np.testing.assert_array_equal(got.euclidean, plain.euclidean)
    assert got.skipped == plain.skipped and got.interpolated == plain.interpolated
    assert got.extras["brightest"] == plain.extras["brightest"] == np.percentile(filt, 99.99)
    assert got.extras["n_template_keypoints"] == plain.extras["n_template_keypoints"]
    np.testing.assert_array_equal(got.aligned.cpu().numpy(), _warped(dev, raw, plain.affines))
    np.testing.assert_array_equal(t.cpu().numpy(), raw)
    # a template given apart from the stack is filtered by the same call
    inp_a, _ = pipeline.detect_slab(t, cfg, template=t[4], prefilter=(S, R))
    inp_b, _ = pipeline.detect_slab(torch.from_numpy(filt).to(dev), cfg, template_index=4)
    assert torch.equal(inp_a.kp_tpl, inp_b.kp_tpl) and torch.equal(inp_a.des_tpl, inp_b.des_tpl)
    assert inp_a.frames.data_ptr() == t.data_ptr()
