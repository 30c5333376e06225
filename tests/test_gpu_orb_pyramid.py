"""The detector's scale pyramid on the device (csrc/resize.hip, kcmc_orb_detect_pyramid in
csrc/orb.hip) against the restatement of tests/test_orb_pyramid_host.py: the resize and
the packed keypoints, descriptors, levels and counts bit-equal; the launcher's batch
loop; the argument errors; and align_images with the "orb_ms" detector and the similarity
model on a stack that zooms."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import test_orb_host as host
import test_orb_pyramid_host as pyr
from conftest import distinct_frames
from kcmc_amd import _lib, orb, stages

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ resize
RESIZE_SHAPES = [((49, 131), (41, 109)), ((160, 200), (133, 167)), ((200, 260), (45, 56)), ((64, 96), (64, 96)),
                 ((96, 130), (48, 65)), ((1, 65535), (1, 54613)), ((7, 5), (3, 2)), ((33, 47), (80, 61))]


@pytest.mark.parametrize("src,dst", RESIZE_SHAPES)
def test_resize_matches_restatement(dev, src, dst):
    img = np.random.default_rng(src[0] * 1000 + src[1]).integers(0, 256, src).astype(np.uint8)
    out = stages.resize_u8(_t(img[None], dev), *dst)
    assert out.shape == (1,) + dst
    assert np.array_equal(out[0].cpu().numpy(), pyr.resize_np(img, *dst))


def test_resize_stack_and_misaligned_view(dev):
    """3 frames with distinct content (a frame stride mistake cannot match), then the same
    stack as a view that starts at an odd byte, into an output that does too."""
    base = host._texture_u8(np.random.default_rng(3), 75, 100)
    imgs = distinct_frames(base, 3)
    want = pyr.resize_np(imgs, 62, 83)
    assert np.array_equal(stages.resize_u8(_t(imgs, dev), 62, 83).cpu().numpy(), want)
    F, H, W = imgs.shape
    for offset in (1, 3):
        buf = torch.zeros(offset + F * H * W + 8, dtype=torch.uint8, device=dev)
        view = buf[offset:offset + F * H * W].view(F, H, W)
        view.copy_(_t(imgs, dev))
        obuf = torch.full((offset + F * 62 * 83 + 8,), 7, dtype=torch.uint8, device=dev)
        out = obuf[offset:offset + F * 62 * 83].view(F, 62, 83)
        assert view.data_ptr() % 4 == offset and out.data_ptr() % 4 == offset
        stages.resize_u8(view, 62, 83, out=out)
        assert np.array_equal(out.cpu().numpy(), want)
        assert (obuf[:offset] == 7).all() and (obuf[offset + F * 62 * 83:] == 7).all()  # nothing outside the output


def test_resize_argument_errors(dev):
    t = torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev)
    for dh, dw in ((0, 4), (4, 0), (65536, 4), (-1, 4)):
        with pytest.raises(ValueError, match="sizes"):
            stages.resize_u8(t, dh, dw)
    with pytest.raises(ValueError, match="contiguous"):
        stages.resize_u8(t[:, :, ::2], 4, 4)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ detection
def _assert_pyramid_matches_oracle(k, f, img, p, tag):
    rkp, rdes, rlvl, counts = pyr.detect_pyramid_oracle(img, p)
    cnt = int(k.count[f].cpu())
    assert cnt == len(rkp), (tag, f, cnt, counts)
    assert np.array_equal(k.kp[f, :cnt].cpu().numpy(), rkp), (tag, f)
    assert np.array_equal(k.des[f, :cnt].cpu().numpy(), rdes), (tag, f)
    assert np.array_equal(k.level[f, :cnt].cpu().numpy(), rlvl), (tag, f)
    return counts


def _detect_case(name):
    """(imgs [F, H, W], OrbParams, the expected per-level counts of frame 0 or None)."""
    q = pyr.QUOTAS_500
    if name in ("cell4", "cell8"):  # the last level under-full: the packing closes a gap
        cell = int(name[4:])
        return pyr.pyramid_case_img(cell)[None], orb.OrbParams(n_levels=8), q[:7] + [pyr.PYR_LAST_COUNT[cell]]
    if name == "thin":  # levels >= 2 fall below 33 rows
        return pyr.thin_img()[None], orb.OrbParams(n_levels=8), None
    if name == "five":  # zero quotas
        return pyr.pyramid_case_img()[None], orb.OrbParams(n_features=5, n_levels=8), [1, 1, 1, 1, 1, 0, 0, 0]
    if name.startswith("levels"):
        return pyr.pyramid_case_img()[None], orb.OrbParams(n_levels=int(name[6:])), None
    if name == "scale1.5":
        return pyr.pyramid_case_img()[None], orb.OrbParams(n_levels=4, scale_factor=1.5), None
    if name == "frames3":
        return distinct_frames(pyr.pyramid_case_img(), 3), orb.OrbParams(n_levels=8), None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["cell4", "cell8", "thin", "five", "levels2", "levels3", "levels8", "scale1.5",
                                  "frames3"])
def test_pyramid_matches_per_level_oracle(dev, name):
    imgs, p, want = _detect_case(name)
    k = stages.detect_orb(_t(imgs, dev), p)
    assert k.level is not None and k.level.shape == (len(imgs), p.n_features) and k.level.dtype == torch.uint8
    assert k.kp.shape == (len(imgs), p.n_features, 2) and k.des.shape == (len(imgs), p.n_features, 32)
    for f in range(len(imgs)):
        counts = _assert_pyramid_matches_oracle(k, f, imgs[f], p, name)
        if f == 0 and want is not None:
            assert counts == want, (name, counts)
    if name == "thin":
        assert counts[1] == 1 and counts[2:] == [0] * 6
    if name == "cell4":  # under-full frames through the matcher's CSR layout: the live rows, in order
        kp, des, q_off, q_off_host = stages.keypoints_csr(k)
        n = sum(counts)
        assert n < p.n_features and q_off_host.tolist() == [0, n] and q_off.cpu().numpy().tolist() == [0, n]
        assert torch.equal(kp, k.kp[0, :n]) and torch.equal(des, k.des[0, :n])


@pytest.mark.parametrize("offset", [1, 3])
def test_pyramid_misaligned_stack(dev, offset):
    """A view that starts at an odd byte with W % 4 == 0: level 0 takes the byte paths, the
    levels in the workspace are aligned again; same result as the aligned stack."""
    imgs = distinct_frames(pyr.pyramid_case_img(), 2)
    F, H, W = imgs.shape
    buf = torch.zeros(offset + F * H * W + 8, dtype=torch.uint8, device=dev)
    view = buf[offset:offset + F * H * W].view(F, H, W)
    view.copy_(_t(imgs, dev))
    assert view.is_contiguous() and view.data_ptr() % 4 == offset and W % 4 == 0
    p = orb.OrbParams(n_levels=8)
    k = stages.detect_orb(view, p)
    for f in range(F):
        _assert_pyramid_matches_oracle(k, f, imgs[f], p, "misaligned")


def test_one_level_is_the_single_scale_entry(dev):
    """n_levels == 1 goes through kcmc_orb_detect: its tensors exactly, and no level column."""
    imgs = _t(distinct_frames(pyr.pyramid_case_img(), 2), dev)
    p = orb.OrbParams(n_features=120)
    k = stages.detect_orb(imgs, orb.OrbParams(n_features=120, n_levels=1, scale_factor=1.7))
    assert k.level is None
    F, N = 2, 120
    kp = torch.full((F, N, 2), -1.0, dtype=torch.float64, device=dev)
    des = torch.full((F, N, 32), 9, dtype=torch.uint8, device=dev)
    cnt = torch.empty((F,), dtype=torch.int32, device=dev)
    pattern, cs = _t(orb.rotated_patterns(), dev), _t(orb.bin_edges(), dev)
    P = ctypes.c_void_p
    _lib.check(_lib.load().kcmc_orb_detect(stages._ctx(dev).handle, P(imgs.data_ptr()), F, 160, 200, p.fast_threshold, N,
                                           p.harris_k, p.edge, P(pattern.data_ptr()), P(cs.data_ptr()),
                                           P(kp.data_ptr()), P(des.data_ptr()), P(cnt.data_ptr()), stages._stream(dev)))
    assert torch.equal(cnt, k.count) and (cnt == N).all()
    assert torch.equal(kp, k.kp) and torch.equal(des, k.des)


def test_pyramid_two_batches(dev):
    """620 frames of 512x512 with 2 levels do not fit the launcher's 1 GiB workspace: the
    second batch mixes batch-local indices (candidate lists, level images, level rows) with
    global ones (outputs)."""
    F, H, W, nf, L = 620, 512, 512, 50, 2
    p = orb.OrbParams(n_features=nf, n_levels=L)
    # kcmc_orb_detect_pyramid's batch size, restated.  If the budget or the per-frame workspace
    # changes so that F frames fit one batch, this test no longer covers the loop: the
    # assertion below then fails, and F must grow.
    sizes = pyr.sizes_np(H, W, L, 1.2)
    ntiles = -(-W // 64) * -(-H // 16)
    slots = ntiles * (64 * 16 // 4)
    per_frame = (2 * slots * (8 + 4) + ntiles * 2 * 4 + 4 + sum(h * w for h, w in sizes[1:]) + nf * (16 + 4 + 32) + 8 * 4)
    batch = min(max(1, min(F, (1 << 30) // per_frame)), 65535)
    assert batch == 610 and F >= batch + 2
    base = _t(host._texture_u8(np.random.default_rng(21), H, W), dev)
    frames = torch.stack([torch.roll(base, (37 * f, 53 * f), (0, 1)) for f in range(F)])
    twin = batch + 5
    frames[twin] = frames[3]  # the same content in both batches
    k = stages.detect_orb(frames, p)
    cnt = k.count.cpu().numpy()
    assert (cnt == nf).all()  # every row is written: whole tensors compare below
    for f in (0, batch - 1, batch, batch + 1, F - 1):
        _assert_pyramid_matches_oracle(k, f, frames[f].cpu().numpy(), p, "two_batches")
    tail = stages.detect_orb(frames[batch:], p)  # the second batch's frames as a first batch
    assert torch.equal(tail.count, k.count[batch:]) and torch.equal(tail.level, k.level[batch:])
    assert torch.equal(tail.kp, k.kp[batch:]) and torch.equal(tail.des, k.des[batch:])
    assert torch.equal(k.kp[twin], k.kp[3]) and torch.equal(k.des[twin], k.des[3]) and torch.equal(k.level[twin], k.level[3])


def test_pyramid_argument_errors(dev):
    """Rejected before any kernel is launched."""
    t = _t(pyr.pyramid_case_img()[None], dev)
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(n_levels=2, scale_factor=1.0),
                dict(n_levels=2, scale_factor=0.8)):
        with pytest.raises(ValueError, match="n_levels|scale_factor"):
            stages.detect_orb(t, orb.OrbParams(**bad))
    with pytest.raises(ValueError, match="edge"):
        stages.detect_orb(t, orb.OrbParams(n_levels=2, edge=15))
    # the C entry's own checks
    P, N = ctypes.c_void_p, 10
    kp = torch.empty((1, N, 2), dtype=torch.float64, device=dev)
    des = torch.empty((1, N, 32), dtype=torch.uint8, device=dev)
    lvl = torch.empty((1, N), dtype=torch.uint8, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    pattern, cs = _t(orb.rotated_patterns(), dev), _t(orb.bin_edges(), dev)

    def call(n_levels, lh, lw, lq):
        lh, lw, lq = (np.array(a, np.int32) for a in (lh, lw, lq))
        return _lib.load().kcmc_orb_detect_pyramid(
            stages._ctx(dev).handle, P(t.data_ptr()), 1, 160, 200, 20, N, 0.04, 16, P(pattern.data_ptr()),
            P(cs.data_ptr()), n_levels, lh.ctypes.data_as(P), lw.ctypes.data_as(P), lq.ctypes.data_as(P),
            P(kp.data_ptr()), P(des.data_ptr()), P(lvl.data_ptr()), P(cnt.data_ptr()), stages._stream(dev))

    def rejected(needle, *a):
        assert call(*a) == _lib.KCMC_EINVAL
        assert needle in _lib.load().kcmc_last_error().decode(), _lib.load().kcmc_last_error()

    assert call(2, [160, 133], [200, 167], [6, 4]) == _lib.KCMC_OK
    rejected("n_levels", 0, [160], [200], [10])
    rejected("n_levels", 9, [160] * 9, [200] * 9, [10] + [0] * 8)
    rejected("sum", 2, [160, 133], [200, 167], [6, 5])
    rejected("sum", 2, [160, 133], [200, 167], [6, 3])
    rejected("non-increasing", 2, [160, 161], [200, 167], [6, 4])
    rejected("non-increasing", 2, [160, 133], [200, 201], [6, 4])
    rejected("non-increasing", 2, [160, 0], [200, 167], [6, 4])
    rejected("level 0", 2, [159, 133], [200, 167], [6, 4])
    rejected("negative", 2, [160, 133], [200, 167], [11, -1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
ZOOMS = (1.2, 1.44, 1.0, 1.0, 1.2, 1.44)   # frame 3 is the template (TEMPLATE_FRAME_LOC = 0.5): zoom 1, no shift
SHIFTS = ((1.5, -2.0), (-2.5, 1.0), (3.0, 2.0), (0.0, 0.0), (-1.0, -3.0), (2.0, 2.5))


def test_align_images_multiscale_similarity_on_a_zooming_stack(dev):
    """6 frames of 240x320 at zoom 1, 1.2 and 1.44 (twice each, small shifts) through
    align_images with "orb_ms" and the similarity model: nothing skipped, every frame's
    scale within 0.5 % of the truth, and the output is the oracle's warp of the returned
    affines."""
    from kcmc_amd import VideoAligner

    class Zoom(VideoAligner):
        RANSAC_MODEL = "similarity"
        DEVICES = [0]

    imgs = np.stack([(pyr.zoom_frame(z, s, noise_seed=i) * 256.0).astype(np.uint16)
                     for i, (z, s) in enumerate(zip(ZOOMS, SHIFTS))])
    va = Zoom()
    aligned, eu, skipped = va.align_images(imgs, n_kp_global=300, detector_algorithm="orb_ms", frame_rate=30)
    truth = np.array([pyr.zoom_truth(z, s) for z, s in zip(ZOOMS, SHIFTS)])
    print("scale", eu[:, 3], "truth", truth[:, 0], "rel", eu[:, 3] / truth[:, 0] - 1)
    print("translation error", eu[:, 0] - truth[:, 1], eu[:, 1] - truth[:, 2])
    assert skipped == []
    assert eu.shape == (6, 4) and aligned.shape == imgs.shape and aligned.dtype == np.uint16
    assert (np.abs(eu[:, 3] / truth[:, 0] - 1) <= 0.005).all(), eu[:, 3] / truth[:, 0] - 1
    for f in range(6):
        assert np.array_equal(aligned[f], oracle.warp_affine_u16(imgs[f], va.affines[f])), f
