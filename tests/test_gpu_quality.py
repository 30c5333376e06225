"""kcmc_amd.quality on the GPU: the two streaming reductions (csrc/quality.hip) and the
VideoAligner switches built on them, against the numpy / Python-integer restatement of
tests/test_quality_host.py.  Every sum is an exact integer, so every comparison is
assert_array_equal."""
import numpy as np
import pytest
import torch

import test_quality_host as host
from kcmc_amd import VideoAligner, quality
from kcmc_amd.video_aligner import GpuOrbDetector
from test_gpu_multidevice import _keypoint_stack

pytestmark = pytest.mark.gpu

# (1, 1, 1): one element; (3, 5, 7): 35 px, not a multiple of 8 (element-wise kernels);
# (67, 33, 130): 67 frames cross a chunk edge, 4290 px; (300, 64, 256): the 16-byte kernels
# (16384 px, W % 8 == 0), several pixel blocks and frame chunks.
SHAPES = [(1, 1, 1), (3, 5, 7), (67, 33, 130), (300, 64, 256)]
_STACKS = {}


def _stack(shape):
    if shape not in _STACKS:
        rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
        x = rng.integers(0, 65536, shape).astype(np.uint16)
        x.reshape(-1)[rng.integers(0, x.size, 3)] = 65535
        _STACKS[shape] = x
    return _STACKS[shape]


# --------------------------------------------------------------------------- stack sum
@pytest.mark.parametrize("shape", SHAPES)
def test_stack_sum_and_mean(dev, shape):
    x = _stack(shape)
    F = shape[0]
    t = torch.from_numpy(x).to(dev)
    rng = np.random.default_rng(5)
    some = rng.random(F) < 0.6
    some[rng.integers(0, F)] = True
    none = np.zeros(F, bool)
    for sel in (None, some):
        s = quality.stack_sum(t, sel)
        assert s.dtype == torch.int64 and tuple(s.shape) == shape[1:]
        np.testing.assert_array_equal(s.cpu().numpy(), host.ref_stack_sum(x, sel))
        m = quality.mean_image(t, sel)
        assert m.dtype == torch.uint16
        np.testing.assert_array_equal(m.cpu().numpy(), host.ref_mean_image(x, sel))
    np.testing.assert_array_equal(quality.stack_sum(t, none).cpu().numpy(), np.zeros(shape[1:], np.int64))
    with pytest.raises(ValueError):
        quality.mean_image(t, none)


def test_stack_sum_of_a_slab_that_starts_mid_allocation(dev):
    x = _stack((7, 33, 41))
    whole = torch.from_numpy(x).to(dev)
    assert whole[3:].data_ptr() % 16 != 0  # 3 frames of 33 x 41 u16 = 8118 bytes in
    np.testing.assert_array_equal(quality.stack_sum(whole[3:]).cpu().numpy(), host.ref_stack_sum(x[3:]))
    y = _stack((6, 3, 12))  # 36 px: the view is 8-byte but not 16-byte aligned, n_px % 8 != 0
    whole = torch.from_numpy(y).to(dev)
    np.testing.assert_array_equal(quality.stack_sum(whole[1:]).cpu().numpy(), host.ref_stack_sum(y[1:]))
    mean = host.ref_mean_image(x[3:])
    np.testing.assert_array_equal(quality.frame_stats(torch.from_numpy(x).to(dev)[3:], mean, (1, 30, 3, 40)),
                                  host.ref_frame_stats(x[3:], mean, (1, 30, 3, 40)).astype(np.int64))


def test_stack_sum_past_32_bits(dev):
    """65540 frames of 65535: every sum is 65535 * 65540 > 2^32, over more than one chunk
    of at most 65536 frames for any chunking."""
    F = 65540
    t = torch.from_numpy(np.full((F, 1, 8), 65535, np.uint16)).to(dev)
    want = np.full((1, 8), 65535 * F, np.int64)
    assert want[0, 0] > 2 ** 32
    np.testing.assert_array_equal(quality.stack_sum(t).cpu().numpy(), want)
    np.testing.assert_array_equal(quality.mean_image(t).cpu().numpy(), np.full((1, 8), 65535, np.uint16))
    sel = np.ones(F, bool)
    sel[::2] = False
    np.testing.assert_array_equal(quality.stack_sum(t, sel).cpu().numpy(), np.full((1, 8), 65535 * (F // 2), np.int64))


def test_stack_sum_over_two_slabs_equals_the_whole(dev):
    x = _stack((67, 33, 130))
    t = torch.from_numpy(x).to(dev)
    a, b = t[:29].clone(), t[29:].clone()
    rng = np.random.default_rng(8)
    sel = rng.random(67) < 0.5
    for s in (None, sel):
        np.testing.assert_array_equal(quality.stack_sum([a, b], s).cpu().numpy(), host.ref_stack_sum(x, s))
        np.testing.assert_array_equal(quality.mean_image([a, b], s).cpu().numpy(), host.ref_mean_image(x, s))
    ref = host.ref_mean_image(x)
    np.testing.assert_array_equal(quality.frame_stats([a, b], ref, (2, 30, 1, 129)),
                                  host.ref_frame_stats(x, ref, (2, 30, 1, 129)).astype(np.int64))


# ------------------------------------------------------------------------- frame stats
def _regions(H, W):
    """The whole image, one pixel, one row, one column, and (where the image has room) a
    rectangle with an odd x0 and an odd width."""
    out = [(0, H, 0, W), (H // 2, H // 2 + 1, W // 2, W // 2 + 1), (H // 3, H // 3 + 1, 0, W), (0, H, W - 1, W)]
    if W >= 7 and H >= 3:
        w = W - 3 if (W - 3) % 2 else W - 4  # the widest odd width from x0 = 3
        out.append((1, H - 1, 3, 3 + w))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_frame_stats(dev, shape):
    x = _stack(shape)
    F, H, W = shape
    ref = np.random.default_rng(21).integers(0, 65536, (H, W)).astype(np.uint16)
    t = torch.from_numpy(x).to(dev)
    regions = _regions(H, W)
    if W >= 7 and H >= 3:
        y0, y1, x0, x1 = regions[-1]
        assert x0 % 2 == 1 and (x1 - x0) % 2 == 1 and x1 <= W
    for region in regions:
        got = quality.frame_stats(t, ref, region)
        assert got.dtype == np.int64 and got.shape == (F, 5)
        np.testing.assert_array_equal(got, host.ref_frame_stats(x, ref, region).astype(np.int64), err_msg=str(region))
        n = (region[1] - region[0]) * (region[3] - region[2])
        np.testing.assert_array_equal(quality.frame_correlations(t, torch.from_numpy(ref).to(dev), region),
                                      host.ref_pearson(got, n))


def test_frame_stats_saturated_frame(dev):
    """All-65535 256 x 256 against all-65535: sum(ab) = 65535^2 * 65536 ~ 2^48."""
    t = torch.from_numpy(np.full((2, 256, 256), 65535, np.uint16)).to(dev)
    got = quality.frame_stats(t, np.full((256, 256), 65535, np.uint16), (0, 256, 0, 256))
    v, n = 65535, 65536
    np.testing.assert_array_equal(got, np.array([[n * v, n * v, n * v * v, n * v * v, n * v * v]] * 2, np.int64))
    assert np.isnan(quality.pearson(got, n)).all()


def test_frame_stats_rejects_bad_rectangles(dev):
    t = torch.from_numpy(_stack((3, 5, 7))).to(dev)
    ref = np.zeros((5, 7), np.uint16)
    for region in [(2, 2, 0, 7), (0, 5, 4, 4), (3, 1, 0, 7), (0, 6, 0, 7), (0, 5, -1, 7)]:
        with pytest.raises(ValueError):
            quality.frame_stats(t, ref, region)
    with pytest.raises(ValueError):
        quality.frame_stats(t, np.zeros((5, 8), np.uint16), (0, 5, 0, 7))


# --------------------------------------------------------------------------- end to end
SCENE_SEED = 31


def _scene(seed=SCENE_SEED):
    """The stack of test_align_images_gpu_detector_split: crops of one noisy scene at
    integer shifts <= 6, the middle frame unshifted."""
    rng = np.random.default_rng(seed)
    H, W, F = 200, 260, 9
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (F, 2))]
    shifts[F // 2] = (0, 0)
    return np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts]), shifts


def _aligner(devices=(0,), metrics=False, refine=0, model="euclidean"):
    class VA(VideoAligner):
        DEVICES = list(devices)
        QUALITY_METRICS = metrics
        TEMPLATE_REFINE_ITERS = refine
        RANSAC_MODEL = model

    return VA()


ATTRS = ("frame_correlations", "mean_image", "valid_region", "template_image", "correlation_history")
KW = dict(n_kp_global=60, detector_algorithm="orb", frame_rate=30)


@pytest.fixture(scope="module")
def runs(dev):
    """Every end-to-end run of the scene, made once: plain, metrics, refined (one and two
    slabs) and the plain run against the restated refined template."""
    imgs, shifts = _scene()
    out = {"imgs": imgs, "shifts": shifts}
    for name, va in (("plain", VideoAligner()), ("off", _aligner()), ("metrics", _aligner(metrics=True)),
                     ("refine", _aligner(refine=1)), ("refine2", _aligner((0, 0), refine=1))):
        out[name] = (va, va.align_images(imgs, **KW))
    return out


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert list(a[2]) == list(b[2])


def test_switches_off_change_nothing(runs):
    _same(runs["off"][1], runs["plain"][1])
    for name in ("plain", "off"):
        for attr in ATTRS:
            assert getattr(runs[name][0], attr) is None, (name, attr)


def test_metrics_equal_the_restatement(runs):
    va, res = runs["metrics"]
    _same(res, runs["plain"][1])
    aligned, eu, skipped = res
    exact = np.array([[[1, 0, dx], [0, 1, dy]] for dy, dx in runs["shifts"]], np.float64)
    print("skipped", skipped, "region", va.valid_region, "max |affines - shifts|", np.abs(va.affines - exact).max(),
          "correlations", va.frame_correlations)
    assert skipped == []  # the premise: every frame has a model of its own
    mean0, region, corr, _ = host.ref_pass_metrics(aligned, va.affines, skipped)
    assert va.valid_region == region == (7, 193, 7, 253)  # max shift 6
    np.testing.assert_array_equal(va.mean_image, mean0)
    assert va.mean_image.dtype == np.uint16
    np.testing.assert_array_equal(va.frame_correlations, corr)
    assert va.frame_correlations.dtype == np.float64 and va.frame_correlations.shape == (len(aligned),)
    assert va.template_image is None and len(va.correlation_history) == 1
    np.testing.assert_array_equal(va.correlation_history[0], corr)
    assert np.nanmin(corr) > 0.9  # registered crops of one scene


def test_refined_pass_equals_a_plain_pass_with_the_restated_template(runs):
    vm, (aligned1, _, skipped1) = runs["metrics"]
    _, _, corr1, sel0 = host.ref_pass_metrics(aligned1, vm.affines, skipped1)
    template = host.ref_refined_template(aligned1, corr1, sel0, 0.5)
    plain = VideoAligner()
    want = plain.align_images(runs["imgs"], masked_template=template, **KW)
    va, res = runs["refine"]
    print("second pass skipped", res[2], "corr", va.correlation_history)
    assert list(res[2]) == []  # the premise: the second pass skips nothing
    _same(res, want)
    np.testing.assert_array_equal(va.template_image, template)
    assert va.template_image.dtype == np.uint16
    assert len(va.correlation_history) == 2
    np.testing.assert_array_equal(va.correlation_history[0], corr1)
    mean2, region2, corr2, _ = host.ref_pass_metrics(res[0], va.affines, res[2])
    np.testing.assert_array_equal(va.correlation_history[1], corr2)
    np.testing.assert_array_equal(va.frame_correlations, corr2)
    np.testing.assert_array_equal(va.mean_image, mean2)
    assert va.valid_region == region2


def test_two_slabs_equal_one_slab_with_refinement(runs):
    (v1, r1), (v2, r2) = runs["refine"], runs["refine2"]
    _same(r2, r1)
    for attr in ("frame_correlations", "mean_image", "template_image"):
        np.testing.assert_array_equal(getattr(v2, attr), getattr(v1, attr), err_msg=attr)
    assert v2.valid_region == v1.valid_region
    assert len(v2.correlation_history) == len(v1.correlation_history) == 2
    for a, b in zip(v2.correlation_history, v1.correlation_history):
        np.testing.assert_array_equal(a, b)


class _HostOrb:
    """The build's detector behind a plain OpenCV-style object: align_images then takes the
    host-detector path (detectAndCompute per frame, _align_detected)."""

    def __init__(self):
        self._d = GpuOrbDetector()

    def detectAndCompute(self, image, mask=None):  # noqa: N802
        return self._d.detectAndCompute(image, mask)


def test_refinement_on_the_host_detector_path(runs):
    def aligner(devices, metrics=False, refine=0):
        class VA(VideoAligner):
            DEVICES = list(devices)
            DETECTOR_CONSTRUCTOR_DICT = {**VideoAligner.DETECTOR_CONSTRUCTOR_DICT, "orb_host": _HostOrb}
            QUALITY_METRICS = metrics
            TEMPLATE_REFINE_ITERS = refine

        return VA()

    imgs = runs["imgs"]
    kw = dict(KW, detector_algorithm="orb_host")
    vm = aligner((0,), metrics=True)
    aligned1, _, skipped1 = vm.align_images(imgs, **kw)
    assert skipped1 == []
    _, _, corr1, sel0 = host.ref_pass_metrics(aligned1, vm.affines, skipped1)
    np.testing.assert_array_equal(vm.frame_correlations, corr1)
    template = host.ref_refined_template(aligned1, corr1, sel0, 0.5)
    want = aligner((0,)).align_images(imgs, masked_template=template, **kw)
    for devices in ((0,), (0, 0)):
        va = aligner(devices, refine=1)
        res = va.align_images(imgs, **kw)
        assert list(res[2]) == []
        _same(res, want)
        np.testing.assert_array_equal(va.template_image, template)
        assert len(va.correlation_history) == 2
        np.testing.assert_array_equal(va.correlation_history[0], corr1)
        np.testing.assert_array_equal(va.correlation_history[1],
                                      host.ref_pass_metrics(res[0], va.affines, res[2])[2])


def test_align_keypoints_metrics(dev):
    ks, frames, kq, dq = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    args = (frames, ks.kp_tpl, ks.des_tpl, kq, dq)
    want = _aligner().align_keypoints(*args, n_kp_global=40)
    for devices in ((0,), (0, 0)):
        va = _aligner(devices, metrics=True)
        res = va.align_keypoints(*args, n_kp_global=40)
        _same(res, want)
        aligned, _, skipped = res
        assert set(skipped) >= {5, 6, 7}  # the premise: frames without a model
        mean0, region, corr, sel0 = host.ref_pass_metrics(aligned, va.affines, skipped)
        assert not set(sel0) & set(skipped) and len(sel0) == len(aligned) - len(skipped)
        np.testing.assert_array_equal(va.mean_image, mean0)  # the mean leaves the skipped frames out
        assert va.valid_region == region
        np.testing.assert_array_equal(va.frame_correlations, corr)
        assert va.frame_correlations.shape == (len(frames),)
    with pytest.raises(ValueError, match="TEMPLATE_REFINE_ITERS"):
        _aligner(refine=1).align_keypoints(*args, n_kp_global=40)
    for kw in (dict(metrics=True), dict(refine=1)):
        with pytest.raises(NotImplementedError):
            _aligner(model="projective", **kw).align_keypoints(*args, n_kp_global=40)
        with pytest.raises(NotImplementedError):
            _aligner(model="projective", **kw).align_images(frames, 40, "orb", 30)
