"""The drop-in VideoAligner over several devices in one process (kcmc_amd.multidevice).

On a one-GPU box the split is rehearsed with a repeated device: DEVICES = [0, 0] puts two
frame slabs on cuda:0, each with its own template copy, match, vote, lookup, RANSAC and
warp; the votes are merged once and the gaps interpolated once on the host.  The returned
arrays must equal DEVICES = [0] (one slab) exactly, with NaN gaps that cross the slab
boundary, temporal downsampling (frame_rate 200: rate 2), the extension models, host and
device inputs, and from raw frames with the GPU detector (normalisation over the split
stack) or a host detector.  One slab and several are one code path (a list of one slab):
the maps a plain run leaves in .affines, more devices than sample frames and a wrong number
of keypoint lists are checked on both."""
import numpy as np
import pytest
import torch

from kcmc_amd import VideoAligner, stages, synthetic

pytestmark = pytest.mark.gpu


def _aligner(devices, model="euclidean"):
    class VA(VideoAligner):
        DEVICES = devices
        RANSAC_MODEL = model

    return VA()


def _keypoint_stack(n_sample, rate, model, blind, seed=61):
    H, W = 96, 160
    ks = synthetic.make_keypoints(n_sample, 150, 32, (H, W), seed=seed, model=model)
    rng = np.random.default_rng(seed)
    for f in blind:  # every descriptor one row: no match passes the ratio test (d1 == d2), no model
        a, b = ks.q_off[f], ks.q_off[f + 1]
        ks.des_q[a:b] = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    base = synthetic.make_texture((H, W), seed=seed)
    frames = np.ascontiguousarray(np.stack([np.roll(base, (2 * f, 5 * f), axis=(0, 1))
                                            for f in range(n_sample * rate - rate // 2)]))
    kq = [ks.kp_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(n_sample)]
    dq = [ks.des_q[ks.q_off[f]:ks.q_off[f + 1]] for f in range(n_sample)]
    return ks, frames, kq, dq


@pytest.mark.parametrize("model,rate,blind", [("euclidean", 1, (5, 6, 7)), ("euclidean", 2, (4, 5)),
                                              ("affine", 1, (0, 1, 6)), ("euclidean", 1, (10, 11)),
                                              ("similarity", 1, (5, 6, 7))])
def test_two_slabs_on_one_gpu_equal_one_slab(dev, model, rate, blind):
    n_sample = 12
    ks, frames, kq, dq = _keypoint_stack(n_sample, rate, model, blind)
    out = {}
    for devices in ([0], [0, 0], [0, 0, 0]):
        va = _aligner(devices, model)
        aligned, eu, skipped = va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40,
                                                  frame_rate=100 * rate)
        out[len(devices)] = (aligned, eu, skipped, va.interpolated_idxs)
    ref = out[1]
    assert isinstance(ref[0], np.ndarray) and ref[0].shape == frames.shape
    assert len(ref[2]) >= len(blind)  # the premise: frames without a model
    for k in (2, 3):
        np.testing.assert_array_equal(out[k][0], ref[0])
        np.testing.assert_array_equal(out[k][1], ref[1])
        assert out[k][2] == ref[2] and out[k][3] == ref[3]


def test_device_input_stays_on_device(dev):
    ks, frames, kq, dq = _keypoint_stack(9, 1, "euclidean", (4,))
    fr = torch.from_numpy(frames).to(dev)
    a1, e1, s1 = _aligner([0]).align_keypoints(fr, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    a2, e2, s2 = _aligner([0, 0]).align_keypoints(fr, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    assert isinstance(a2, torch.Tensor) and a2.device == fr.device
    assert torch.equal(a1, a2) and s1 == s2
    np.testing.assert_array_equal(e1, e2)


def test_brightest_px_over_parts_equals_whole(dev):
    rng = np.random.default_rng(9)
    x = rng.integers(0, 65536, (7, 33, 41)).astype(np.uint16)
    x[2, 3, 4] = 65535
    whole = torch.from_numpy(x).to(dev)
    parts = [whole[:3], whole[3:3], whole[3:]]
    b = stages.brightest_px(parts)
    assert b == stages.brightest_px(whole) == np.percentile(x, 99.99)
    # a slab that starts mid-allocation (3 frames of 33 x 41 u16 = 8118 bytes in): the
    # 16-byte kernels work on an aligned copy
    assert whole[3:].data_ptr() % 16 != 0
    np.testing.assert_array_equal(stages.max_scale_u8(whole[3:], b).cpu().numpy(), stages.max_scale_lut(b)[x[3:]])


def test_align_images_gpu_detector_split(dev):
    """align_images from raw uint16 frames with the GPU detector: the percentile of the
    split stack from the summed per-device histograms, detection per slab; identical to
    one slab."""
    rng = np.random.default_rng(31)
    H, W, F = 200, 260, 9
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (F, 2))]
    shifts[F // 2] = (0, 0)
    imgs = np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts])
    a1, e1, s1 = _aligner([0]).align_images(imgs, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
    a2, e2, s2 = _aligner([0, 0]).align_images(imgs, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
    assert s1 == s2 == []
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(e1, e2)
    np.testing.assert_allclose(e2[:, 0], [dx for dy, dx in shifts], atol=1e-6)


@pytest.fixture(scope="module")
def plain_runs(dev):
    """align_keypoints with no switch on, one slab and two, and a second call of each instance
    on another stack."""
    first = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    second = _keypoint_stack(9, 1, "euclidean", (2,), seed=62)
    runs = {}
    for devices in ((0,), (0, 0)):
        va = _aligner(list(devices))
        for name, (ks, frames, kq, dq) in (("first", first), ("second", second)):
            aligned, _, skipped = va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
            runs[devices, name] = (frames, aligned, skipped, va.affines)
    return runs


@pytest.mark.parametrize("call", ["first", "second"])
def test_plain_run_leaves_its_maps(plain_runs, call):
    """No switch on: .affines holds the maps of the call -- a row per frame, the same from one
    slab and from two, and every returned frame is the oracle's warp of its source with its row
    -- also after an earlier call of the same instance on a longer stack."""
    import oracle

    frames, aligned, skipped, affines = plain_runs[(0,), call]
    _, aligned2, skipped2, affines2 = plain_runs[(0, 0), call]
    assert skipped and skipped == skipped2  # the premise: interpolated maps among them
    assert affines.shape == (len(frames), 2, 3) and not np.isnan(affines).any()
    np.testing.assert_array_equal(affines2, affines)
    np.testing.assert_array_equal(aligned2, aligned)
    for f in range(len(frames)):
        assert np.array_equal(aligned[f], oracle.warp_affine_u16(frames[f], affines[f])), f


class _HostOrb:
    """The build's detector behind a plain OpenCV-style object: align_images takes the
    host-detector path (detectAndCompute per frame)."""

    def __init__(self):
        from kcmc_amd.video_aligner import GpuOrbDetector

        self._d = GpuOrbDetector()

    def detectAndCompute(self, image, mask=None):  # noqa: N802
        return self._d.detectAndCompute(image, mask)


def test_align_images_host_detector_split(dev):
    """align_images with a host detector, a masked_template and a patch: one slab, two slabs
    and a device-tensor input give the same returns, the last as a tensor on its device."""
    rng = np.random.default_rng(32)
    H, W, F = 160, 200, 7
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (F, 2))]
    imgs = np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts])
    template = scene[16:16 + H, 16:16 + W].copy()
    template[:, :24] = 0  # masked: no keypoints from the left margin
    kw = dict(n_kp_global=60, detector_algorithm="orb_host", frame_rate=30, masked_template=template,
              patch=(10, 20, 100, 120))

    def run(devices, images):
        class VA(VideoAligner):
            DEVICES = devices
            DETECTOR_CONSTRUCTOR_DICT = {**VideoAligner.DETECTOR_CONSTRUCTOR_DICT, "orb_host": _HostOrb}

        va = VA()
        return va.align_images(images, **kw), va

    (a1, e1, s1), v1 = run([0], imgs)
    assert isinstance(a1, np.ndarray) and a1.shape == (F, 100, 120) and s1 == []
    np.testing.assert_allclose(e1[:, 0], [dx for dy, dx in shifts], atol=1e-6)
    dev_imgs = torch.from_numpy(imgs).to(dev)
    for devices, images in (([0, 0], imgs), ([0], dev_imgs), ([0, 0], dev_imgs)):
        (a, e, s), va = run(devices, images)
        if isinstance(images, torch.Tensor):
            assert isinstance(a, torch.Tensor) and a.device == images.device
            a = a.cpu().numpy()
        np.testing.assert_array_equal(a, a1)
        np.testing.assert_array_equal(e, e1)
        assert s == s1 and va.interpolated_idxs == v1.interpolated_idxs
        np.testing.assert_array_equal(va.affines, v1.affines)
    np.testing.assert_array_equal(dev_imgs.cpu().numpy(), imgs)  # the caller's tensor is not written


def test_more_devices_than_sample_frames(dev, monkeypatch):
    """Empty slabs are dropped: four devices for three sample frames equal one device, and a
    one-frame stack on two devices is one slab, which takes the one-slab hot call."""
    ks, frames, kq, dq = _keypoint_stack(3, 1, "euclidean", ())
    want = _aligner([0]).align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    got = _aligner([0, 0, 0, 0]).align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    assert want[0].shape == frames.shape
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)

    ks, frames, kq, dq = _keypoint_stack(1, 1, "euclidean", ())
    assert len(frames) == 1
    want = _aligner([0]).align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)

    def no_split(*args, **kwargs):
        raise AssertionError("one slab must not take the split hot path")

    from kcmc_amd import multidevice

    monkeypatch.setattr(multidevice, "align_split", no_split)
    got = _aligner([0, 0]).align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_wrong_number_of_keypoint_lists(dev, devices):
    ks, frames, kq, dq = _keypoint_stack(6, 1, "euclidean", ())
    with pytest.raises(ValueError, match=r"keypoints must be given for every sample frame images\[::rate\]"):
        _aligner(devices).align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq[:-1], dq[:-1], n_kp_global=40)
