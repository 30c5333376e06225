"""The bicubic warp on the device (csrc/warp_cubic.hip) against the numpy restatement of
tests/test_warp_cubic_host.py, bit for bit: sizes at the kernel's seams, every map family (staged,
border, direct gather, zeros, saturating, NaN), the three kinds of content, unaligned slabs, a
seeded sweep, and the switch end to end through VideoAligner."""
import math

import numpy as np
import pytest
import torch

from conftest import distinct_frames
from kcmc_amd import VideoAligner, quality, stages
from test_warp_cubic_host import checkerboard, random_u16, ref_warp_affine_cubic, rot_about_centre, shift_map

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD
# 1 x 1, 3 x 5: never interior; 4 x 4: one interior pixel at most; 57 x 129: odd W, two tile rows,
# a one-column last tile; 64 x 130: tile64, W % 8 != 0 but even, a two-column last tile; 56 x 128:
# exactly one tile; 65 x 131: both odd, partial tiles both ways; 128 x 264: W % 8 == 0 (16-byte
# staging), tile64, three tile columns
SIZES = [(1, 1), (3, 5), (4, 4), (57, 129), (64, 130), (56, 128), (65, 131), (128, 264)]


def inverse_maps(H, W):
    """(name, inverse map) of every family; the warp reads source (M (x, y, 1))."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    maps = [("identity", shift_map(0, 0)), ("shift+3-2", shift_map(3, -2)), ("shift-5+7", shift_map(-5, 7))]
    maps += [(f"fx{k}", shift_map(1 + k / 32.0, 0.25)) for k in range(32)]
    maps += [(f"fy{k}", shift_map(-0.75, k / 32.0 - 2)) for k in range(32)]
    maps.append(("rot0.02", rot_about_centre(0.02, H, W, 0.3, -0.6)))
    maps.append(("rot90", rot_about_centre(math.pi / 2, H, W, 0.4, 0.1)))
    maps.append(("scale3", np.array([[3.0, 0, -2 * cx + 0.2], [0, 3.0, -2 * cy - 0.3]])))
    maps.append(("scale0.3", np.array([[0.3, 0, 0.7 * cx], [0, 0.3, 0.7 * cy + 0.1]])))
    maps.append(("out", shift_map(W + 5, 0.5)))
    maps.append(("out-y", shift_map(0.5, -(H + 7))))
    for k in (1, 2, 3):  # a k-pixel strip stays in, whole-pixel and half-pixel
        maps.append((f"strip{k}x", shift_map(W - k, 0)))
        maps.append((f"strip{k}x.5", shift_map(-(W - k) + 0.5, 0.25)))
        maps.append((f"strip{k}y", shift_map(0.5, H - k - 0.5)))
        maps.append((f"strip{k}y-", shift_map(0, -(H - k))))
    maps.append(("far+", shift_map(40000.3, -40000.7)))
    maps.append(("far-", shift_map(-41234.5, 45000.25)))
    return maps


def forward_maps(H, W):
    """Forward maps (inverted on the device as OpenCV inverts them)."""
    return [("identity", shift_map(0, 0)), ("shift", shift_map(2.40625, -1.71875)),
            ("rot0.02", rot_about_centre(0.02, H, W, -0.3, 0.6)), ("rot-0.02", rot_about_centre(-0.02, H, W, 1.5, 2.5)),
            ("rot90", rot_about_centre(math.pi / 2, H, W)), ("scale3", rot_about_centre(0.1, H, W, scale=3.0)),
            ("scale0.3", rot_about_centre(-0.05, H, W, scale=0.3)), ("singular", np.zeros((2, 3))),
            ("far", shift_map(-40000.3, 40000.7))]


def with_nan(M):
    """A NaN map between two valid ones."""
    M = np.array(M, np.float64)
    if len(M) >= 3:
        M[len(M) // 2, 1, 0] = np.nan
    return M


def content(kind, H, W, F, seed=0):
    if kind == "random":
        fr = distinct_frames(random_u16(H, W, seed + 7 * H + W), F)
        fr[:, H // 2, W // 2] = 65535
        return fr
    if kind == "checker":
        return distinct_frames(checkerboard(H, W), F)  # rolled by odd amounts: every frame its own phase
    assert kind == "bright"
    return np.full((F, H, W), 65535, np.uint16)


def run_cubic(dev, frames, M, inverse_map):
    """One call on its own buffers: the output pre-filled with a sentinel between guard frames,
    the source compared after the call."""
    F, H, W = frames.shape
    src = torch.from_numpy(frames).to(dev)
    buf = torch.full((F + 2, H, W), SENTINEL, dtype=torch.uint16, device=dev)
    got = stages.warp_affine_u16(src, torch.from_numpy(np.ascontiguousarray(M, np.float64)).to(dev), out=buf[1:F + 1],
                                 inverse_map=inverse_map, interpolation="cubic")
    assert got.data_ptr() == buf[1:].data_ptr()
    b = buf.cpu().numpy()
    assert (b[0] == SENTINEL).all() and (b[F + 1] == SENTINEL).all()
    np.testing.assert_array_equal(src.cpu().numpy(), frames)
    return b[1:F + 1]


def check(dev, frames, named_maps, inverse_map):
    M = np.stack([m for _, m in named_maps])
    got = run_cubic(dev, frames, M, inverse_map)
    want = ref_warp_affine_cubic(frames, M, inverse_map)
    for f, (name, _) in enumerate(named_maps):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"frame {f}: map {name}")
    return got


# ------------------------------------------------------------------ every size, every map family
@pytest.mark.parametrize("H,W", SIZES)
def test_every_map_family_is_the_restatement(dev, H, W):
    named = inverse_maps(H, W)
    mid = len(named) // 2
    named = named[:mid] + [("nan", with_nan(np.stack([shift_map(0, 0)] * 3))[1])] + named[mid:]
    frames = content("random", H, W, len(named))
    got = check(dev, frames, named, inverse_map=True)
    names = [n for n, _ in named]
    np.testing.assert_array_equal(got[names.index("identity")], frames[names.index("identity")])
    for n in ("out", "out-y", "far+", "far-", "nan"):
        assert (got[names.index(n)] == 0).all(), n
    if H > 8 and W > 8:
        k = names.index("shift+3-2")
        np.testing.assert_array_equal(got[k][2:, :W - 3], frames[k][:H - 2, 3:])
        assert (got[k][:2] == 0).all() and (got[k][:, W - 3:] == 0).all()
        for n in ("strip1x", "strip2x.5", "strip3y", "strip1y-"):
            assert got[names.index(n)].any(), n


@pytest.mark.parametrize("H,W", SIZES)
def test_forward_maps_are_the_restatement(dev, H, W):
    named = forward_maps(H, W)
    M = with_nan(np.stack([m for _, m in named]))
    named = [(n, m) for (n, _), m in zip(named, M)]
    check(dev, content("random", H, W, len(named), seed=1), named, inverse_map=False)


CLAMP_SIZES = [(4, 4), (57, 129), (64, 130), (128, 264)]


def clamp_maps(H, W):
    return [(n, m) for n, m in inverse_maps(H, W) if n[0] == "f" or n.startswith(("rot", "scale", "strip", "ident"))]


@pytest.mark.parametrize("kind", ["checker", "bright"])
@pytest.mark.parametrize("H,W", CLAMP_SIZES)
def test_clamping_content_is_the_restatement(dev, kind, H, W):
    named = clamp_maps(H, W)
    frames = content(kind, H, W, len(named))
    got = check(dev, frames, named, inverse_map=True)
    if kind == "checker" and H > 8:
        k = [n for n, _ in named].index("fx16")  # half a pixel: both clamps
        assert (got[k][4:-4, 4:-4] == 0).any() and (got[k][4:-4, 4:-4] == 65535).any()
    check(dev, frames[:len(forward_maps(H, W))], forward_maps(H, W), inverse_map=False)


# ------------------------------------------------------------------ unaligned slabs
VIEW_SIZES = [(57, 129), (64, 136), (65, 130)]
VIEW_OFFSETS = ((1, 1), (0, 1), (1, 0), (1, 8))  # (source, output) elements into their buffers


def view_maps(H, W):
    return [(n, m) for n, m in inverse_maps(H, W) if n in ("identity", "fx7", "fy21", "rot0.02", "rot90", "strip2x.5")]


@pytest.mark.parametrize("H,W", VIEW_SIZES)
def test_views_one_element_into_a_buffer(dev, H, W):
    """A source slab and an output that start 1 element into their buffers: element-wise staging
    (also at W % 8 == 0) and the unpaired store (also at even W)."""
    named = view_maps(H, W)
    F = len(named)
    frames = content("random", H, W, F, seed=5)
    M = np.stack([m for _, m in named])
    want = ref_warp_affine_cubic(frames, M, inverse_map=True)
    n = F * H * W
    sflat = torch.zeros(n + 9, dtype=torch.uint16, device=dev)
    sflat[1:1 + n] = torch.from_numpy(frames.reshape(-1)).to(dev)
    oflat = torch.full((n + 9,), SENTINEL, dtype=torch.uint16, device=dev)
    Md = torch.from_numpy(M).to(dev)
    for s_off, o_off in VIEW_OFFSETS:
        oflat.fill_(SENTINEL)
        if s_off == 0:
            src = torch.from_numpy(frames).to(dev)
        else:
            src = sflat[1:1 + n].view(F, H, W)
            assert src.data_ptr() % 16 == 2 or src.data_ptr() % 4 == 2
        out = oflat[o_off:o_off + n].view(F, H, W)
        stages.warp_affine_u16(src, Md, out=out, inverse_map=True, interpolation="cubic")
        o = oflat.cpu().numpy()
        np.testing.assert_array_equal(o[o_off:o_off + n].reshape(F, H, W), want)
        assert (o[:o_off] == SENTINEL).all() and (o[o_off + n:] == SENTINEL).all()
        np.testing.assert_array_equal(src.cpu().numpy(), frames)


# ------------------------------------------------------------------ a seeded sweep
def sweep_cases():
    """(case, H, W, content kind, inverse_map, map family, maps [3, 2, 3]) of the seeded sweep."""
    rng = np.random.default_rng(20240607)
    for case in range(40):
        H, W = int(rng.integers(1, 201)), int(rng.integers(1, 261))
        kind = ("random", "checker", "bright")[int(rng.integers(0, 3))]
        inv = bool(rng.integers(0, 2))
        fam = int(rng.integers(0, 5))
        F = 3
        Ms = []
        for _ in range(F):
            if fam == 0:
                Ms.append(shift_map(rng.uniform(-8, 8), rng.uniform(-8, 8)))
            elif fam == 1:
                Ms.append(rot_about_centre(rng.uniform(-0.03, 0.03), H, W, rng.uniform(-4, 4), rng.uniform(-4, 4)))
            elif fam == 2:
                Ms.append(rot_about_centre(rng.uniform(-math.pi, math.pi), H, W, rng.uniform(-20, 20),
                                           rng.uniform(-20, 20), scale=rng.uniform(0.25, 4.0)))
            elif fam == 3:
                Ms.append(shift_map(rng.integers(-W - 2, W + 3) + rng.integers(0, 32) / 32.0,
                                    rng.integers(-H - 2, H + 3) + rng.integers(0, 32) / 32.0))
            else:
                Ms.append(np.array([[rng.uniform(0.9, 1.1), rng.uniform(-0.1, 0.1), rng.uniform(-6, 6)],
                                    [rng.uniform(-0.1, 0.1), rng.uniform(0.9, 1.1), rng.uniform(-6, 6)]]))
        yield case, H, W, kind, inv, fam, np.stack(Ms)


def test_seeded_sweep_of_random_cases(dev):
    for case, H, W, kind, inv, fam, M in sweep_cases():
        frames = content(kind, H, W, len(M), seed=case)
        got = run_cubic(dev, frames, M, inv)
        np.testing.assert_array_equal(got, ref_warp_affine_cubic(frames, M, inv),
                                      err_msg=f"case {case}: {H} x {W}, {kind}, family {fam}, inverse_map {inv}")


# ------------------------------------------------------------------ arguments
def test_arguments(dev):
    fr = torch.zeros((2, 8, 8), dtype=torch.uint16, device=dev)
    M = torch.from_numpy(np.stack([shift_map(0, 0)] * 2)).to(dev)
    with pytest.raises(ValueError):
        stages.warp_affine_u16(fr, M, interpolation="lanczos")
    with pytest.raises(NotImplementedError):
        stages.warp_affine_u16(torch.zeros((2, 8, 8, 3), dtype=torch.uint16, device=dev), M, interpolation="cubic")
    with pytest.raises(ValueError):  # in place
        stages.warp_affine_u16(fr, M, out=fr, interpolation="cubic")
    empty = stages.warp_affine_u16(fr[:0], M[:0], interpolation="cubic")
    assert empty.shape == (0, 8, 8)


# ------------------------------------------------------------------ end to end
def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), **kw})()


@pytest.fixture(scope="module")
def e2e(dev):
    """A 12-frame 96 x 160 synthetic stack with three frames without a model, run once per aligner."""
    from test_gpu_multidevice import _keypoint_stack

    ks, frames, kq, dq = _keypoint_stack(12, 1, "euclidean", (5, 6, 7))
    out = {"frames": frames}
    for name, va in (("cubic", _va(WARP_INTERPOLATION="cubic")), ("cubic2", _va((0, 0), WARP_INTERPOLATION="cubic")),
                     ("linear", _va(WARP_INTERPOLATION="linear")), ("plain", _va()),
                     ("linear_metrics", _va(WARP_INTERPOLATION="linear", QUALITY_METRICS=True))):
        out[name] = (va, va.align_keypoints(frames, ks.kp_tpl, ks.des_tpl, kq, dq, n_kp_global=40))
    return out


def test_end_to_end_frames_are_the_cubic_warp_of_the_sources(e2e):
    frames = e2e["frames"]
    va, (aligned, eu, skipped) = e2e["cubic"]
    assert aligned.shape == frames.shape and aligned.dtype == np.uint16
    assert va.affines is not None and np.isfinite(va.affines[:len(frames)]).all()
    for f in range(len(frames)):
        np.testing.assert_array_equal(aligned[f], ref_warp_affine_cubic(frames[f], va.affines[f]), err_msg=str(f))
    assert len(skipped) >= 3 and len(va.interpolated_idxs) >= 3  # the premise: frames warped again on the host's maps
    frac = np.abs(va.affines[:len(frames), :, 2] * 32 - np.rint(va.affines[:len(frames), :, 2] * 32))
    assert (frac > 1e-3).any()  # and maps off the whole pixel: the weights are at work


def test_end_to_end_everything_but_the_frames_is_the_linear_runs(e2e):
    va_c, (a_c, eu_c, sk_c) = e2e["cubic"]
    va_l, (a_l, eu_l, sk_l) = e2e["linear"]
    va_m, (a_m, eu_m, sk_m) = e2e["linear_metrics"]
    np.testing.assert_array_equal(eu_c, eu_l)
    assert list(sk_c) == list(sk_l) and va_c.interpolated_idxs == va_l.interpolated_idxs
    np.testing.assert_array_equal(va_c.affines, va_m.affines)
    np.testing.assert_array_equal(a_m, a_l)
    assert (a_c != a_l).any()
    # "linear" is the class that never sets the attribute
    _, (a_p, eu_p, sk_p) = e2e["plain"]
    np.testing.assert_array_equal(a_l, a_p)
    np.testing.assert_array_equal(eu_l, eu_p)
    assert list(sk_l) == list(sk_p)


def test_end_to_end_two_slabs_equal_one(e2e):
    va1, (a1, eu1, sk1) = e2e["cubic"]
    va2, (a2, eu2, sk2) = e2e["cubic2"]
    np.testing.assert_array_equal(a2, a1)
    np.testing.assert_array_equal(eu2, eu1)
    np.testing.assert_array_equal(va2.affines, va1.affines)
    assert list(sk2) == list(sk1) and va2.interpolated_idxs == va1.interpolated_idxs


def test_apply_affine_follows_the_switch(dev):
    img = random_u16(57, 129, 4)
    M = rot_about_centre(0.01, 57, 129, 1.3, -0.4)
    got = _va(WARP_INTERPOLATION="cubic")._apply_affine(img, M)
    np.testing.assert_array_equal(got, ref_warp_affine_cubic(img, M))
    assert (VideoAligner._apply_affine(img, M) != got).any()


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
@pytest.mark.parametrize("mode", ["metrics", "fallback", "refine"])
def test_end_to_end_with_the_intensity_passes(dev, mode, devices):
    """Once each with QUALITY_METRICS, FALLBACK = "correlation" and REFINE = "intensity" (the
    metrics on in every run: they publish valid_region): the final frames are the cubic warp of
    the sources under the final affines, and the region is the taps = 4 rectangle."""
    from test_gpu_refine import _e2e_stack

    e = _e2e_stack(blind=True)
    kw = {"metrics": {}, "fallback": dict(FALLBACK="correlation"), "refine": dict(REFINE="intensity")}[mode]
    va = _va(devices, WARP_INTERPOLATION="cubic", QUALITY_METRICS=True, **kw)
    aligned, eu, skipped = va.align_keypoints(e["frames"], e["kp_tpl"], e["des_tpl"], e["kq"], e["dq"], n_kp_global=40)
    n, (H, W) = len(e["frames"]), e["frames"].shape[1:]
    for f in range(n):
        np.testing.assert_array_equal(aligned[f], ref_warp_affine_cubic(e["frames"][f], va.affines[f]), err_msg=str(f))
    assert tuple(va.valid_region) == quality.valid_region(va.affines[:n], H, W, taps=4)
    y0, y1, x0, x1 = quality.valid_region(va.affines[:n], H, W)
    assert tuple(va.valid_region) == (y0 + 1, y1 - 1, x0 + 1, x1 - 1)
    assert len(skipped) == 1  # the premise: the blind frame
    if mode == "fallback":
        assert va.fallback_idxs == list(skipped)  # the pass ran and re-warped the blind frame
    if mode == "refine":
        assert va.refine_steps is not None and len(va.refine_idxs) > 0


# ------------------------------------------------------------------ every path with 2 x 3 maps
def _slab(dev, F, H, W, seed, blind=()):
    from kcmc_amd import pipeline, synthetic

    ks = synthetic.make_keypoints(F, 150, 32, (H, W), seed=seed)
    rng = np.random.default_rng(seed)
    for f in blind:  # no match passes the ratio test: no model, a second warp with the host's map
        ks.des_q[ks.q_off[f]:ks.q_off[f + 1]] = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    frames = distinct_frames(synthetic.make_texture((H, W), seed=seed), F)
    return frames, pipeline.SlabInputs(torch.from_numpy(frames).to(dev), torch.from_numpy(ks.des_tpl).to(dev),
                                       torch.from_numpy(ks.kp_tpl).to(dev), torch.from_numpy(ks.des_q).to(dev),
                                       torch.from_numpy(ks.kp_q).to(dev), torch.from_numpy(ks.q_off).to(dev), ks.q_off)


def test_config_switch_on_every_pipeline_path(dev):
    """align_slab, OverlappedSlabs (both schedules), align_streamed and align_split with
    warp_interpolation = "cubic": the restatement's frames under the linear run's maps."""
    from kcmc_amd import multidevice, pipeline

    F, H, W = 14, 96, 160
    frames, inp = _slab(dev, F, H, W, seed=41, blind=(0, 6, 7))
    cubic = pipeline.AlignConfig(n_kp_global=40, warp_interpolation="cubic")
    lin = pipeline.align_slab(inp, pipeline.AlignConfig(n_kp_global=40))
    ref = pipeline.align_slab(inp, cubic)
    assert len(ref.skipped) == 3
    np.testing.assert_array_equal(ref.affines, lin.affines)
    want = ref_warp_affine_cubic(frames, ref.affines[:F])
    np.testing.assert_array_equal(ref.aligned.cpu().numpy(), want)
    assert (want != lin.aligned.cpu().numpy()).any()
    for beside in (False, True):
        ov = pipeline.OverlappedSlabs(dev, cubic, match_beside=beside)
        assert ov.submit(inp) is None
        (got,) = ov.flush()
        ov.synchronize()
        np.testing.assert_array_equal(got.aligned.cpu().numpy(), want)
        assert got.skipped == ref.skipped
    out, res = pipeline.align_streamed(torch.from_numpy(frames).pin_memory(), inp, cubic, slab=5)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.numpy(), want)
    np.testing.assert_array_equal(res.affines, ref.affines)
    # two slabs of one stack through the split path's stage table (warp_params, then warp for
    # the frames without a model)
    ranges = multidevice.split_frames(F, 1, 2)
    parts = multidevice.split_to_devices(frames, ranges, [0, 0])
    kp_q, des_q, q_off = inp.kp_q.cpu().numpy(), inp.des_q.cpu().numpy(), inp.q_off_host
    slabs = multidevice.make_slabs(parts, ranges, inp.des_tpl.cpu().numpy(), inp.kp_tpl.cpu().numpy(), kp_q, des_q,
                                   q_off)
    sp = multidevice.align_split(slabs, ranges, cubic)
    np.testing.assert_array_equal(torch.cat(sp.aligned).cpu().numpy(), want)
    np.testing.assert_array_equal(sp.affines, ref.affines)
