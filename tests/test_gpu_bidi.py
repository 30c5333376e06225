"""kcmc_amd.bidi on the GPU: the phase-sums and row-shift kernels (csrc/bidi_phase.hip) against
the numpy restatement of tests/test_bidi_host.py, bit for bit -- sizes at the kernels' seams,
every radius and shift, indexing, slab views off the 16-byte grid, guard frames, in place and
out of place -- and the switch end to end through VideoAligner."""
import ctypes

import numpy as np
import pytest
import torch

from kcmc_amd import VideoAligner, _lib, bidi
from test_bidi_host import check_validation, fast_bidi_sums, random_u16, ref_bidi_sums, ref_shift_rows

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD


def ints(a):
    return [[[int(v) for v in e] for e in row] for row in a]


# ------------------------------------------------------------------------------ phase sums
# (2, 17): one row pair, one column at R = 8; (3, 33): one column at R = 16, an odd row with both
# neighbours; (33, 41): odd W, the last odd row has both; (57, 129): odd H; (64, 136): W % 8 == 0, the
# 16-byte path, the last odd row has one neighbour; (65, 130): even W off the vector grid
SUM_SIZES = [(2, 17), (3, 33), (33, 41), (57, 129), (64, 136), (65, 130)]


@pytest.mark.parametrize("H,W", SUM_SIZES)
def test_sums_are_the_restatement_at_every_radius(dev, H, W):
    x = random_u16((3, H, W), 11 * H + W)
    x[1, H // 2, W // 2] = 65535
    t = torch.from_numpy(x).to(dev)
    for R in (0, 1, 8, 16):
        if W < 2 * R + 1:
            with pytest.raises(ValueError, match="W must"):
                bidi.phase_sums(t, [0], R)
            continue
        got = bidi.phase_sums(t, [0, 1, 2], R)
        assert got.shape == (3, 2 * R + 1, 5) and got.dtype == np.int64
        np.testing.assert_array_equal(got, fast_bidi_sums(x, R), err_msg=f"R = {R}")
        if R in (0, 8):  # the fast restatement is the sample-by-sample one (host test); once more here
            assert ints(got[:1]) == ints(ref_bidi_sums(x, [0], R))
    np.testing.assert_array_equal(t.cpu().numpy(), x)


@pytest.mark.parametrize("H,W", [(64, 136), (57, 129)])
def test_sums_of_an_all_bright_frame(dev, H, W):
    """All 65535: the largest sums the shapes allow, every narrower partial sum at its bound."""
    x = np.full((2, H, W), 65535, np.uint16)
    for R in (8, 16):
        got = bidi.phase_sums(torch.from_numpy(x).to(dev), [0, 1], R)
        n = bidi.sample_count(H, W, R)
        want = np.array([n * 65535, n * 65535, n * 65535 ** 2, n * 65535 ** 2, n * 65535 ** 2], np.int64)
        assert (got == want).all()
        off, r, ok = bidi.estimate_offset(got, n)
        assert (off, ok) == (0, False) and np.isnan(r).all()


def test_sums_over_several_tiles_and_workgroups(dev):
    """A row longer than one staged tile (1024 columns) on both paths, and more odd rows than a
    frame gets workgroups when many frames are selected."""
    for H, W in ((5, 2600), (4, 2091)):
        x = random_u16((1, H, W), W)
        np.testing.assert_array_equal(bidi.phase_sums(torch.from_numpy(x).to(dev), [0], 16), fast_bidi_sums(x, 16))
    x = random_u16((2, 41, 24), 5)
    idx = [0, 1] * 600  # 1200 selected: fewer workgroups per frame than odd rows
    got = bidi.phase_sums(torch.from_numpy(x).to(dev), idx, 3)
    np.testing.assert_array_equal(got, fast_bidi_sums(x, 3)[idx])


def test_sums_indexing_and_slab_views(dev):
    """frame_idx NULL, repeated, unordered and out of range; two slabs that are views of one
    allocation, the second off the 16-byte grid."""
    H, W, R = 33, 41, 2
    x = random_u16((5, H, W), 41)
    want = fast_bidi_sums(x, R)
    t = torch.from_numpy(x).to(dev)
    # NULL frame_idx through the C ABI: frames 0 .. n_sel - 1
    out = torch.full((3, 2 * R + 1, 5), -1, dtype=torch.int64, device=dev)
    ctx = _lib.context(0).handle
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().kcmc_bidi_phase_sums_u16(ctx, ctypes.c_void_p(t.data_ptr()), 5, H, W, None, 3, R,
                                                    ctypes.c_void_p(out.data_ptr()), stream))
    np.testing.assert_array_equal(out.cpu().numpy(), want[:3])
    slabs = [t[:2], t[2:]]
    assert slabs[0].data_ptr() % 16 == 0 and slabs[1].data_ptr() % 16 == 4 and slabs[1].is_contiguous()
    idx = [4, 0, 4, 7, -1, 2]
    got = bidi.phase_sums(slabs, idx, R)
    assert got.shape == (6, 5, 5)
    np.testing.assert_array_equal(got[[0, 1, 2, 5]], want[[4, 0, 4, 2]])
    assert not got[3].any() and not got[4].any() and got[0].any()
    np.testing.assert_array_equal(got, bidi.phase_sums(t, idx, R))
    # the 16-byte path and the element path give one answer: a view one frame into a W % 8 == 0 stack
    y = random_u16((3, 9, 24), 3)  # 9 * 24 * 2 bytes per frame: frame 1 starts on the grid, so shift by one element
    flat = torch.from_numpy(np.concatenate([[0], y.reshape(-1)]).astype(np.uint16)).to(dev)
    view = flat[1:].view(3, 9, 24)
    assert view.data_ptr() % 16 == 2
    np.testing.assert_array_equal(bidi.phase_sums(view, [0, 1, 2], 4), fast_bidi_sums(y, 4))
    assert bidi.phase_sums(t, [], R).shape == (0, 5, 5)


def test_sums_recover_a_planted_offset_on_the_device(dev):
    from test_bidi_host import planted

    x = planted(57, 129, -4, 2000)
    idx = bidi.sample_indices(len(x), 64)
    off, r, ok = bidi.estimate_offset(bidi.phase_sums(torch.from_numpy(x).to(dev), idx, 8), bidi.sample_count(57, 129, 8))
    assert (off, ok) == (-4, True)


def test_entry_points_validate_with_device_pointers(dev):
    fr = torch.zeros((2, 33, 40), dtype=torch.uint16, device=dev)
    dst = torch.zeros((1, 33, 40), dtype=torch.uint16, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros((1, 17, 5), dtype=torch.int64, device=dev)
    check_validation(_lib.context(0).handle, (fr.data_ptr(), idx.data_ptr(), out.data_ptr(), dst.data_ptr()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- row shift
# (1, 1), (2, 3), (3, 5): narrower than the shift; (57, 129), (65, 130): the element path; (64, 136): the
# 16-byte path; (4, 2600): a thread owns more than one vector; (2, 32767): the longest row;
# (2, 32760), (2, 32728): W % 8 == 0 above and at the longest row the padded LDS image holds
SHIFT_SIZES = [(1, 1), (2, 3), (3, 5), (57, 129), (64, 136), (65, 130), (4, 2600), (2, 32767), (2, 32760), (2, 32728)]
SHIFTS = [-16, -9, -8, -1, 0, 1, 7, 8, 16]


def guarded(dev, x, offset=0):
    """x between two sentinel guard frames in one buffer that starts ``offset`` elements into its
    allocation: (the buffer, the view of x)."""
    F, H, W = x.shape
    n = H * W
    buf = torch.full(((F + 2) * n + offset,), SENTINEL, dtype=torch.uint16, device=dev)
    view = buf[offset + n:offset + (F + 1) * n].view(F, H, W)
    view.copy_(torch.from_numpy(x).to(dev))
    return buf, view


def guards_intact(buf, x, offset=0):
    F, H, W = x.shape
    n = H * W
    b = buf.cpu().numpy()
    return (b[:offset + n] == SENTINEL).all() and (b[offset + (F + 1) * n:] == SENTINEL).all()


@pytest.mark.parametrize("H,W", SHIFT_SIZES)
def test_shift_rows_is_the_restatement(dev, H, W):
    F = 2 if W > 30000 else 3
    x = random_u16((F, H, W), 3 * H + W)
    src = torch.from_numpy(x).to(dev)
    for parity in (0, 1):
        for d in SHIFTS:
            want = ref_shift_rows(x, d, parity)
            # out of place, into a sentinel-filled buffer between guard frames
            buf, out = guarded(dev, np.full_like(x, SENTINEL))
            got = bidi.shift_rows(src, d, parity, out=out)
            assert got.data_ptr() == out.data_ptr()
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"out of place: parity {parity}, d {d}")
            assert guards_intact(buf, x)
            # in place, between guard frames
            buf, view = guarded(dev, x)
            got = bidi.shift_rows(view, d, parity, out=view)
            assert got.data_ptr() == view.data_ptr()
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"in place: parity {parity}, d {d}")
            assert guards_intact(buf, x)
    np.testing.assert_array_equal(src.cpu().numpy(), x)  # the source of the out-of-place calls
    fresh = bidi.shift_rows(src, 5)  # out=None: a new tensor, odd rows
    assert fresh.data_ptr() != src.data_ptr()
    np.testing.assert_array_equal(fresh.cpu().numpy(), ref_shift_rows(x, 5, 1))


@pytest.mark.parametrize("H,W", [(6, 24), (5, 13), (64, 136)])
def test_shift_rows_on_views_one_element_into_their_buffers(dev, H, W):
    """Source and output start one element into their allocations (off the 16-byte grid), each
    alone and both; the 16-byte and the element path give one answer."""
    x = random_u16((3, H, W), H + W)
    for so, do in ((1, 0), (0, 1), (1, 1)):
        for d in (-9, -1, 0, 8, 3):
            sbuf, src = guarded(dev, x, so)
            dbuf, dst = guarded(dev, np.full_like(x, SENTINEL), do)
            assert src.data_ptr() % 16 == (2 * (so + H * W)) % 16
            got = bidi.shift_rows(src, d, 1, out=dst)
            np.testing.assert_array_equal(got.cpu().numpy(), ref_shift_rows(x, d, 1), err_msg=f"{so} {do} {d}")
            np.testing.assert_array_equal(src.cpu().numpy(), x)
            assert guards_intact(dbuf, x, do) and guards_intact(sbuf, x, so)
    buf, view = guarded(dev, x, 1)  # in place on such a view
    np.testing.assert_array_equal(bidi.shift_rows(view, -7, 0, out=view).cpu().numpy(), ref_shift_rows(x, -7, 0))
    assert guards_intact(buf, x, 1)


def test_shift_rows_slabs_arguments_and_overlap(dev):
    x = random_u16((5, 12, 40), 9)
    t = torch.from_numpy(x).to(dev)
    slabs = [t[:2], t[2:]]
    got = bidi.shift_rows(slabs, 4)
    assert isinstance(got, list) and len(got) == 2
    np.testing.assert_array_equal(torch.cat(got).cpu().numpy(), ref_shift_rows(x, 4))
    np.testing.assert_array_equal(t.cpu().numpy(), x)
    own = [s.clone() for s in slabs]
    same = bidi.shift_rows(own, -2, out=own)  # in place per slab
    assert [o.data_ptr() for o in same] == [o.data_ptr() for o in own]
    np.testing.assert_array_equal(torch.cat(own).cpu().numpy(), ref_shift_rows(x, -2))
    flat = torch.zeros(2 * x.size, dtype=torch.uint16, device=dev)
    a = flat[:x.size].view(x.shape)
    a.copy_(t)
    for off in (1, 40, 12 * 40, x.size - 1):  # partial overlap is refused, nothing is written
        b = flat[off:off + x.size].view(x.shape)
        with pytest.raises(ValueError, match="overlap"):
            bidi.shift_rows(a, 1, out=b)
        with pytest.raises(ValueError, match="overlap"):
            bidi.shift_rows(b, 1, out=a)
    np.testing.assert_array_equal(a.cpu().numpy(), x)
    for bad in (17, -17, 1.5, True, "1"):
        with pytest.raises(ValueError):
            bidi.shift_rows(t, bad)
    with pytest.raises(ValueError):
        bidi.shift_rows(t, 1, parity=2)
    with pytest.raises(ValueError):
        bidi.shift_rows(t, 1, out=t[:4])
    with pytest.raises(TypeError):
        bidi.shift_rows(t.to(torch.int16), 1)
    assert bidi.shift_rows(t[:0], 3).shape == (0, 12, 40)


# ------------------------------------------------------------------------------ end to end
def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), **kw})()


def _run_kp(va, frames, ks, kq, dq):
    aligned, eu, skipped = va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    if isinstance(aligned, torch.Tensor):
        aligned = aligned.cpu().numpy()
    return dict(aligned=aligned, eu=eu, skipped=list(skipped), affines=va.affines,
                interpolated=list(va.interpolated_idxs))


def assert_same_run(got, want, what=""):
    np.testing.assert_array_equal(got["aligned"], want["aligned"], err_msg=what)
    np.testing.assert_array_equal(got["eu"], want["eu"], err_msg=what)
    assert got["skipped"] == want["skipped"] and got["interpolated"] == want["interpolated"], what
    if want["affines"] is None:
        assert got["affines"] is None, what
    else:
        np.testing.assert_array_equal(got["affines"], want["affines"], err_msg=what)


@pytest.fixture(scope="module")
def e2e(dev):
    """The 12-frame 96 x 160 stack of tests/test_gpu_warp_cubic.py's fixture (three frames without a
    model); ``planted``: the same stack with the odd rows displaced by 3."""
    from test_gpu_multidevice import _keypoint_stack

    ks, frames, kq, dq = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    return dict(ks=ks, frames=frames, kq=kq, dq=dq, planted=ref_shift_rows(frames, -3))


@pytest.mark.parametrize("kw", [{}, dict(REFINE="intensity"), dict(WARP_INTERPOLATION="cubic"),
                                dict(FALLBACK="correlation", QUALITY_METRICS=True)],
                         ids=["plain", "refine", "cubic", "fallback+metrics"])
def test_fixed_offset_is_the_plain_aligner_on_the_shifted_stack(dev, e2e, kw):
    ks, frames, kq, dq = e2e["ks"], e2e["frames"], e2e["kq"], e2e["dq"]
    want = _run_kp(_va(**kw), ref_shift_rows(frames, 3), ks, kq, dq)
    va = _va(BIDI_PHASE=3, **kw)
    got = _run_kp(va, frames, ks, kq, dq)
    assert_same_run(got, want)
    assert (va.bidi_offset, va.bidi_correlations, va.bidi_frames, va.bidi_accepted) == (3, None, [], True)
    assert len(want["skipped"]) >= 3  # the premise: frames warped again on the host's maps
    assert (got["aligned"] != _run_kp(_va(**kw), frames, ks, kq, dq)["aligned"]).any()
    assert_same_run(_run_kp(_va((0, 0), BIDI_PHASE=3, **kw), frames, ks, kq, dq), want, "two slabs")


def test_auto_finds_the_planted_offset(dev, e2e):
    ks, kq, dq, stack = e2e["ks"], e2e["kq"], e2e["dq"], e2e["planted"]
    want = _run_kp(_va(BIDI_PHASE=3), stack, ks, kq, dq)
    for devices in ((0,), (0, 0)):
        va = _va(devices, BIDI_PHASE="auto", BIDI_PHASE_FRAMES=5)
        got = _run_kp(va, stack, ks, kq, dq)
        assert va.bidi_offset == 3 and va.bidi_accepted is True
        assert va.bidi_frames == bidi.sample_indices(12, 5) == [0, 2, 5, 8, 11]
        assert va.bidi_correlations.shape == (17,) and int(np.nanargmax(va.bidi_correlations)) == 8 + 3
        assert_same_run(got, want, str(devices))
    one, two = _va((0,), BIDI_PHASE="auto"), _va((0, 0), BIDI_PHASE="auto")
    _run_kp(one, stack, ks, kq, dq), _run_kp(two, stack, ks, kq, dq)
    np.testing.assert_array_equal(one.bidi_correlations, two.bidi_correlations)  # per-slab sums add exactly
    assert one.bidi_frames == list(range(12))
    # a clean stack: the peak is at 0, accepted, nothing moves
    va = _va(BIDI_PHASE="auto")
    clean = _run_kp(va, e2e["frames"], ks, kq, dq)
    assert (va.bidi_offset, va.bidi_accepted) == (0, True)
    assert_same_run(clean, _run_kp(_va(), e2e["frames"], ks, kq, dq))
    # the switch off again: the results are reset
    va.BIDI_PHASE = "none"
    _run_kp(va, e2e["frames"], ks, kq, dq)
    assert va.bidi_offset is None and va.bidi_correlations is None and va.bidi_frames is None
    assert va.bidi_accepted is None


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_a_device_tensor_input_is_never_written(dev, e2e, devices):
    ks, frames, kq, dq = e2e["ks"], e2e["frames"], e2e["kq"], e2e["dq"]
    t = torch.from_numpy(frames).to(dev)
    aligned, eu, skipped = _va(devices, BIDI_PHASE=3).align_keypoints(t, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40)
    assert isinstance(aligned, torch.Tensor)
    np.testing.assert_array_equal(t.cpu().numpy(), frames)
    want = _run_kp(_va(devices), ref_shift_rows(frames, 3), ks, kq, dq)
    np.testing.assert_array_equal(aligned.cpu().numpy(), want["aligned"])
    np.testing.assert_array_equal(eu, want["eu"])


def _scene_stack():
    """The stack of tests/test_gpu_multidevice.py's align_images test: 9 shifted crops of a blocky
    scene, 200 x 260."""
    rng = np.random.default_rng(3)
    H, W, F = 200, 260, 9
    lo = rng.integers(0, 60000, (H // 4 + 8, W // 4 + 8)).astype(np.float64)
    scene = np.clip(np.kron(lo, np.ones((4, 4))) + rng.normal(0, 800, (H + 32, W + 32)), 0, 65535).astype(np.uint16)
    shifts = [(int(a), int(b)) for a, b in rng.integers(-6, 7, (F, 2))]
    shifts[F // 2] = (0, 0)
    return np.stack([scene[16 + dy:16 + dy + H, 16 + dx:16 + dx + W] for dy, dx in shifts])


def test_align_images_takes_its_template_from_the_corrected_stack(dev):
    """align_images with the GPU detector, host and device input, one slab and two: everything
    downstream -- normalisation, detection, the template frame, the warp -- reads the corrected
    stack, so the run equals the plain aligner's on the stack shifted beforehand."""
    imgs = _scene_stack()
    shifted = ref_shift_rows(imgs, -2)

    def run(va, x):
        aligned, eu, skipped = va.align_images(x, n_kp_global=60, detector_algorithm="orb", frame_rate=30)
        aligned = aligned.cpu().numpy() if isinstance(aligned, torch.Tensor) else aligned
        return dict(aligned=aligned, eu=eu, skipped=list(skipped), affines=None,
                    interpolated=list(va.interpolated_idxs))

    want = run(_va(), shifted)
    assert np.isfinite(want["eu"]).all() and len(want["skipped"]) < len(imgs) // 2
    for devices in ((0,), (0, 0)):
        assert_same_run(run(_va(devices, BIDI_PHASE=-2), imgs), want, f"host input, {devices}")
        t = torch.from_numpy(imgs).to(dev)
        assert_same_run(run(_va(devices, BIDI_PHASE=-2), t), want, f"device input, {devices}")
        np.testing.assert_array_equal(t.cpu().numpy(), imgs)
    # a masked_template is used as given
    tpl = shifted[len(imgs) // 2]
    va = _va(BIDI_PHASE=-2)
    a1 = va.align_images(imgs, 60, "orb", 30, masked_template=tpl)
    a0 = _va().align_images(shifted, 60, "orb", 30, masked_template=tpl)
    np.testing.assert_array_equal(a1[0], a0[0])
    np.testing.assert_array_equal(a1[1], a0[1])
