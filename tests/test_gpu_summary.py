"""kcmc_amd.summary on the GPU: the temporal-sums reduction (csrc/temporal_sums.hip) and the
VideoAligner switch built on it, against the numpy / Python-integer restatement of
tests/test_summary_host.py.  Every sum is an exact integer and the finishing functions round
each term once, so every comparison is assert_array_equal."""
import numpy as np
import pytest
import torch

import test_quality_host as qhost
import test_summary_host as host
from kcmc_amd import VideoAligner, _lib, quality, stages, summary
from test_gpu_multidevice import _keypoint_stack
from test_gpu_quality import KW, _same, _scene

pytestmark = pytest.mark.gpu

# (H, W, rectangle): 5 x 8 whole -- the 16-byte path; 9 x 24 with the rectangle's edges inside a
# vector; 7 x 13 whole and inside -- the element path; 12 x 40 a wider 16-byte case with
# mid-vector edges.  (Tiles are 16 rows x 128 columns: tests of more than one tile are
# test_more_than_one_tile and the sweep.)
CASES = [(5, 8, (0, 5, 0, 8)), (9, 24, (1, 8, 3, 21)), (7, 13, (0, 7, 0, 13)), (7, 13, (2, 6, 1, 12)),
         (12, 40, (2, 11, 3, 37))]
FRAMES = [1, 2, 33, 70]  # chunks of at least 32 frames: 1, 1, 2 and 3 of them
GUARD, GUARD_I64, GUARD_U16 = 64, -0x0123456789ABCDEF, 0xABCD
_STACKS = {}


def _stack(F, H, W):
    if (F, H, W) not in _STACKS:
        rng = np.random.default_rng(F * 1000003 + H * 1009 + W)
        x = rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
        x.reshape(-1)[rng.integers(0, x.size, 3)] = 65535
        _STACKS[(F, H, W)] = x
    return _STACKS[(F, H, W)]


def entry(t, region, sel, neighbours, dev):
    """kcmc_temporal_sums_u16 itself on the device tensor ``t`` as it is (aligned or not), into
    the middle of sentinel-filled buffers: (planes, max) as numpy arrays, after checking that
    every sentinel survived -- with H * W odd, the one straight after the max image too."""
    F, H, W = t.shape
    K = 2 + neighbours // 2
    pbuf = torch.full((2 * GUARD + K * H * W,), GUARD_I64, dtype=torch.int64, device=dev)
    mbuf = torch.full((2 * GUARD + H * W,), GUARD_U16, dtype=torch.uint16, device=dev)
    planes, top = pbuf[GUARD:GUARD + K * H * W], mbuf[GUARD:GUARD + H * W]
    s = None if sel is None else torch.from_numpy(np.ascontiguousarray(sel).view(np.uint8)).to(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kcmc_temporal_sums_u16(
            stages._ctx(dev).handle, stages._ptr(t), F, H, W, stages._ptr(s), *(int(v) for v in region), neighbours,
            stages._ptr(planes), stages._ptr(top), stages._stream(dev)))
    p, m = pbuf.cpu().numpy(), mbuf.cpu().numpy()
    assert (p[:GUARD] == GUARD_I64).all() and (p[-GUARD:] == GUARD_I64).all(), "a sentinel beside the planes changed"
    assert (m[:GUARD] == GUARD_U16).all() and (m[-GUARD:] == GUARD_U16).all(), "a sentinel beside the max changed"
    return p[GUARD:-GUARD].reshape(K, H, W), m[GUARD:-GUARD].reshape(H, W)


def _check(got, want):
    n, planes, top = got
    wn, wplanes, wtop = want
    assert n == wn
    planes, top = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (planes, top))
    assert planes.dtype == np.int64 and top.dtype == np.uint16
    np.testing.assert_array_equal(planes, wplanes)
    np.testing.assert_array_equal(top, wtop)


# ----------------------------------------------------------------------- the reduction
@pytest.mark.parametrize("neighbours", [4, 8])
@pytest.mark.parametrize("F", FRAMES)
@pytest.mark.parametrize("H,W,region", CASES)
def test_temporal_sums(dev, H, W, region, F, neighbours):
    x = _stack(F, H, W)
    t = torch.from_numpy(x).to(dev)
    want = host.ref_temporal_sums(x, region, None, neighbours)
    got = summary.temporal_sums(t, region, None, neighbours)
    assert tuple(got[1].shape) == (2 + neighbours // 2, H, W) and tuple(got[2].shape) == (H, W)
    _check(got, want)
    assert t.data_ptr() % 16 == 0  # the 16-byte path when W % 8 == 0
    _check((F,) + entry(t, region, None, neighbours, dev), want)


@pytest.mark.parametrize("neighbours", [4, 8])
def test_more_than_one_tile(dev, neighbours):
    """35 x 264 and 19 x 261: three tiles down and three across (16 rows x 128 columns each), on
    the 16-byte and on the element path, rectangle edges inside a tile and inside a vector."""
    for H, W, region in ((35, 264, (0, 35, 0, 264)), (35, 264, (1, 34, 5, 259)), (19, 261, (0, 19, 2, 261))):
        x = _stack(37, H, W)
        _check(summary.temporal_sums(torch.from_numpy(x).to(dev), region, None, neighbours),
               host.ref_temporal_sums(x, region, None, neighbours))


def test_selection(dev):
    H, W, region = 9, 24, (1, 8, 3, 21)
    x = _stack(70, H, W)
    t = torch.from_numpy(x).to(dev)
    runs = np.ones(70, bool)
    runs[3:9] = runs[31:40] = runs[64:] = False  # runs of unselected frames, across the chunk edges
    runs[1] = False
    odd = np.arange(70) % 2 == 1
    for sel in (runs, odd):
        for nb in (4, 8):
            _check(summary.temporal_sums(t, region, sel, nb), host.ref_temporal_sums(x, region, sel, nb))
    none = np.zeros(70, bool)
    n, planes, top = summary.temporal_sums(t, region, none)
    assert n == 0 and not planes.cpu().numpy().any() and not top.cpu().numpy().any()
    planes, top = entry(t, region, none, 8, dev)
    assert not planes.any() and not top.any()
    for bad in (np.ones(69, bool), np.ones(70, np.uint8)):
        with pytest.raises(ValueError):
            summary.temporal_sums(t, region, bad)


def test_no_frames_gives_zeros(dev):
    t = torch.zeros((0, 5, 8), dtype=torch.uint16, device=dev)
    planes, top = entry(t, (0, 5, 0, 8), None, 8, dev)
    assert not planes.any() and not top.any()


def test_slab_that_starts_mid_allocation(dev):
    """A view whose base is not 16-byte aligned takes the element path although W % 8 == 0: the C
    entry on the view as it is (the wrapper would copy it to an aligned buffer first)."""
    for H, W, region, skip in ((9, 24, (1, 8, 3, 21), 3), (5, 8, (0, 5, 0, 8), 1), (7, 13, (2, 6, 1, 12), 2)):
        x = _stack(33, H, W)
        flat = torch.from_numpy(np.concatenate([np.zeros(skip, np.uint16), x.reshape(-1)])).to(dev)
        view = flat[skip:].view(33, H, W)
        assert view.data_ptr() % 16 == 2 * skip
        for nb in (4, 8):
            want = host.ref_temporal_sums(x, region, None, nb)
            _check((33,) + entry(view, region, None, nb, dev), want)
            _check(summary.temporal_sums(view, region, None, nb), want)
    whole = torch.from_numpy(_stack(7, 33, 41)).to(dev)  # 3 frames of 33 x 41 u16 = 8118 bytes in
    assert whole[3:].data_ptr() % 16 != 0
    _check(summary.temporal_sums(whole[3:], (1, 30, 3, 40)),
           host.ref_temporal_sums(_stack(7, 33, 41)[3:], (1, 30, 3, 40)))


@pytest.mark.parametrize("F", [65537, 65540])
def test_past_one_chunk_of_frames_and_32_bits(dev, F):
    """F frames of 2 x 8 pixels, all 65535: more than one chunk of at most 65536 frames for any
    chunking.  65537 frames reach sum a = 65535 * 65537 = 2^32 - 1, the largest value of a 32-bit
    accumulator; 65540 frames pass 2^32.  Every expected value is a closed form."""
    v = 65535
    t = torch.full((F, 2, 8), v, dtype=torch.uint16, device=dev)
    assert 65537 * v == 2 ** 32 - 1 and 65540 * v > 2 ** 32
    for nb in (4, 8):
        n, planes, top = summary.temporal_sums(t, (0, 2, 0, 8), None, nb)
        planes, top = planes.cpu().numpy(), top.cpu().numpy()
        assert n == F
        np.testing.assert_array_equal(planes[0], np.full((2, 8), F * v, np.int64))
        np.testing.assert_array_equal(planes[1], np.full((2, 8), F * v * v, np.int64))
        sq = F * v * v
        right = np.full((2, 8), sq, np.int64)
        right[:, 7] = 0
        np.testing.assert_array_equal(planes[2], right)
        down = np.zeros((2, 8), np.int64)
        down[0] = sq
        np.testing.assert_array_equal(planes[3], down)
        if nb == 8:
            dr, dl = down.copy(), down.copy()
            dr[0, 7] = 0
            dl[0, 0] = 0
            np.testing.assert_array_equal(planes[4], dr)
            np.testing.assert_array_equal(planes[5], dl)
        np.testing.assert_array_equal(top, np.full((2, 8), v, np.uint16))
    sel = np.ones(F, bool)
    sel[::2] = False
    n, planes, _ = summary.temporal_sums(t, (0, 2, 0, 8), sel, 4)
    assert n == F // 2
    np.testing.assert_array_equal(planes[1].cpu().numpy(), np.full((2, 8), (F // 2) * v * v, np.int64))


def test_two_slabs_equal_the_whole(dev):
    H, W, region = 12, 40, (2, 11, 3, 37)
    x = _stack(70, H, W)
    t = torch.from_numpy(x).to(dev)
    a, b = t[:29].clone(), t[29:].clone()
    sel = np.random.default_rng(8).random(70) < 0.5
    for s in (None, sel):
        for nb in (4, 8):
            want = host.ref_temporal_sums(x, region, s, nb)
            _check(summary.temporal_sums([a, b], region, s, nb), want)
            _check(summary.temporal_sums(t, region, s, nb), want)
    # the max of a pixel lives in one slab only
    y = x.copy()
    y[:29, 5, 20], y[29:, 5, 20] = 7, 3
    y[:29, 6, 21], y[29:, 6, 21] = 40000, 65535  # above 32767: the order of uint16, not int16
    parts = [torch.from_numpy(y[:29]).to(dev), torch.from_numpy(y[29:]).to(dev)]
    _check(summary.temporal_sums(parts, region), host.ref_temporal_sums(y, region))


def test_rejects_bad_arguments(dev):
    t = torch.from_numpy(_stack(2, 5, 8)).to(dev)
    for region in [(2, 2, 0, 8), (0, 5, 4, 4), (3, 1, 0, 8), (0, 6, 0, 8), (0, 5, -1, 8)]:
        with pytest.raises(ValueError):
            summary.temporal_sums(t, region)
    for nb in (6, 0, 16):
        with pytest.raises(ValueError):
            summary.temporal_sums(t, (0, 5, 0, 8), None, nb)


# --------------------------------------------------------------------------- end to end
def _aligner(devices=(0,), on=False, neighbours=8, interpolation="linear"):
    class VA(VideoAligner):
        DEVICES = list(devices)
        SUMMARY_IMAGES = on
        SUMMARY_NEIGHBOURS = neighbours
        WARP_INTERPOLATION = interpolation

    return VA()


ATTRS = host.ATTRS


def _check_attributes(va, aligned, region, neighbours=8):
    want = host.ref_summary(np.asarray(aligned), region, neighbours)
    assert va.summary_region == region
    for name, w in want.items():
        got = getattr(va, name)
        np.testing.assert_array_equal(got, w, err_msg=name)
        if name != "crispness":
            assert got.dtype == w.dtype and got.shape == w.shape, name
    assert isinstance(va.crispness, float) and va.crispness > 0


@pytest.fixture(scope="module")
def runs(dev):
    """Every end-to-end run of the scene, made once."""
    imgs, shifts = _scene()
    # independent noise per frame: without it the registered crops of one scene are identical
    # inside the valid region, every temporal variance is 0 and every correlation NaN
    noise = np.random.default_rng(77).normal(0, 300, imgs.shape)
    imgs = np.clip(imgs + noise, 0, 65535).astype(np.uint16)
    out = {"imgs": imgs, "shifts": shifts}
    for name, va in (("plain", VideoAligner()), ("off", _aligner()), ("on", _aligner(on=True)),
                     ("on2", _aligner((0, 0), on=True)), ("on4", _aligner(on=True, neighbours=4)),
                     ("cubic", _aligner(on=True, interpolation="cubic"))):
        out[name] = (va, va.align_images(imgs, **KW))
    return out


def test_switch_off_changes_nothing(runs):
    _same(runs["off"][1], runs["plain"][1])
    for name in ("plain", "off"):
        for attr in ATTRS:
            assert getattr(runs[name][0], attr) is None, (name, attr)
    for name in ("on", "on2", "on4"):  # ... and with it on, what is returned stays what it was
        _same(runs[name][1], runs["plain"][1])
        for attr in ("frame_correlations", "mean_image", "valid_region", "template_image", "correlation_history"):
            assert getattr(runs[name][0], attr) is None, (name, attr)


def test_attributes_equal_the_restatement(runs):
    va, (aligned, _, skipped) = runs["on"]
    assert skipped == []
    H, W = aligned.shape[1:]
    region = qhost.ref_valid_region(va.affines[:len(aligned)], H, W)
    assert region[0] >= 7 and region[2] >= 7  # max shift 6
    _check_attributes(va, aligned, region)
    y0, y1, x0, x1 = region
    inside = va.correlation_image[y0:y1, x0:x1]
    print("region", region, "crispness", va.crispness, "mean local correlation", np.nanmean(inside),
          "mean std", va.std_image[y0:y1, x0:x1].mean())
    assert np.isfinite(inside).all() and (va.std_image[y0:y1, x0:x1] > 0).all()  # the premise: nothing degenerate
    assert np.isnan(va.correlation_image[:y0]).all() and np.isnan(va.std_image[:, :x0]).all()
    assert not va.max_image[:y0].any() and not va.summary_mean_image[:, x1:].any()
    assert (va.max_image >= va.summary_mean_image).all()


def test_four_neighbours_two_slabs_and_cubic(runs):
    va4, (aligned, _, _) = runs["on4"]
    _check_attributes(va4, aligned, runs["on"][0].summary_region, neighbours=4)
    v1, v2 = runs["on"][0], runs["on2"][0]
    assert v2.summary_region == v1.summary_region and v2.crispness == v1.crispness
    for attr in ("summary_mean_image", "max_image", "std_image", "correlation_image"):
        np.testing.assert_array_equal(getattr(v2, attr), getattr(v1, attr), err_msg=attr)
    vc, (aligned_c, _, skipped) = runs["cubic"]
    assert skipped == []
    H, W = aligned_c.shape[1:]
    region = quality.valid_region(vc.affines[:len(aligned_c)], H, W, taps=4)
    lin = qhost.ref_valid_region(vc.affines[:len(aligned_c)], H, W)
    assert region == (lin[0] + 1, lin[1] - 1, lin[2] + 1, lin[3] - 1)  # one more pixel for the 4 x 4 footprint
    _check_attributes(vc, aligned_c, region)


def test_attributes_are_reset_by_the_next_call(runs, dev):
    va = _aligner(on=True)
    va.align_images(runs["imgs"], **KW)
    assert va.crispness is not None
    type(va).SUMMARY_IMAGES = False
    va.align_images(runs["imgs"], **KW)
    for attr in ATTRS:
        assert getattr(va, attr) is None, attr


def test_align_keypoints_summary(dev):
    ks, frames, kq, dq = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    args = (frames, ks.kp_tpl, ks.des_tpl, kq, dq)
    want = _aligner().align_keypoints(*args, n_kp_global=40)
    for devices in ((0,), (0, 0)):
        va = _aligner(devices, on=True)
        res = va.align_keypoints(*args, n_kp_global=40)
        _same(res, want)
        aligned, _, skipped = res
        assert set(skipped) >= {5, 6, 7}  # frames without a model are part of the stack all the same
        H, W = aligned.shape[1:]
        _check_attributes(va, aligned, qhost.ref_valid_region(va.affines[:len(aligned)], H, W))
