"""kcmc_amd.refine_field on the GPU: the tile gradient-sums kernel (csrc/refine_tiles.hip)
against the numpy restatement of tests/test_refine_field_host.py and against the existing
kcmc_gradient_sums_u16, bit for bit, and the VideoAligner switch built on it, end to end.
Every sum is an exact integer, so every kernel comparison is assert_array_equal."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import test_refine_field_host as host
from kcmc_amd import VideoAligner, _lib, refine, refine_field
from kcmc_amd.stages import _ctx

pytestmark = pytest.mark.gpu

F = 3


def _frames(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 65536, shape).astype(np.uint16)
    x.reshape(-1)[rng.integers(0, x.size, 5)] = 65535
    return x


def _raw(dev, frames_t, idx, n_sel, ref_t, rows, cols):
    """The entry point itself (``idx``: a list, or None for the NULL index list): [n_sel, ty,
    tx, 5] int64.  The output starts as -1 everywhere: the call writes every entry."""
    n_frames, H, W = frames_t.shape
    r, c = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    ty, tx = len(r) - 1, len(c) - 1
    out = torch.full((n_sel, ty, tx, 5), -1, dtype=torch.int64, device=dev)
    idx_t = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=dev)
    P = ctypes.c_void_p
    _lib.check(_lib.load().kcmc_tile_gradient_sums_u16(
        _ctx(dev).handle, P(frames_t.data_ptr()), n_frames, H, W, None if idx is None else P(idx_t.data_ptr()), n_sel,
        P(ref_t.data_ptr()), r.ctypes.data_as(P), ty, c.ctypes.data_as(P), tx, P(out.data_ptr()),
        P(torch.cuda.current_stream(dev).cuda_stream)))
    return out.cpu().numpy()


def _five(dev, t, idx, ref_t, rect):
    """The first five of kcmc_gradient_sums_u16's sums over ``rect``, its bands added (int64:
    these five stay below 2^63 over a rectangle of fewer than 2^31 pixels)."""
    got = refine.gradient_sums(t, idx, ref_t, rect)
    return np.array([[int(v) for v in row[:5]] for row in got], np.int64).reshape(len(idx), 5)


def _limit(lo, hi):
    """33 edges of 32 tiles in [lo, hi]: one pixel each, the last takes the rest."""
    e = lo + np.arange(33)
    e[-1] = hi
    return e.tolist()


# (H, W, tilings (rows, cols)).  40 x 72: the 16-byte path, 8 thread columns x 32 row groups in two
# chunks; 37 x 61: W % 8 != 0, the element path.  Per shape: edges off the multiples of 8 with a
# one-pixel-wide tile, an empty tile, a one-row tile row and an empty tile row; one tile; 32 x 32
# tiles.  20 x 520: 64 thread columns, a wave per row segment; 12 x 2064: 258 vectors in 9 chunks
# of 32 thread columns; 7 x 2056: 256 thread columns, four waves along a row.
CASES = [
    (40, 72, [((1, 7, 7, 19, 20, 39), (1, 5, 13, 14, 14, 37, 71)), ((3, 37), (5, 67)), (_limit(1, 39), _limit(1, 71)),
              ((11, 11), (1, 71)), ((1, 39), (9, 9, 9))]),
    (37, 61, [((1, 9, 18, 27, 36), (1, 10, 20, 21, 21, 50, 60)), ((4, 33), (6, 47)), (_limit(1, 36), _limit(1, 60))]),
    (20, 520, [((2, 9, 18), (9, 70, 71, 300, 515))]),
    (12, 2064, [((1, 4, 11), (3, 500, 1027, 1028, 2061))]),
    (7, 2056, [((1, 6), (8, 511, 513, 1030, 2055)), ((2, 3, 5), (1, 2055))]),
]


@pytest.mark.parametrize("H,W,tilings", CASES)
def test_tile_sums_equal_the_restatement_and_the_existing_kernel(dev, H, W, tilings):
    x = _frames((F, H, W), H * 1000 + W)
    ref = _frames((H, W), 77 + W)
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    assert (t.data_ptr() | ref_t.data_ptr()) % 16 == 0
    for rows, cols in tilings:
        want = host.ref_tile_sums(x, [0, 1, 2], ref, list(rows), list(cols))
        got = _raw(dev, t, [0, 1, 2], F, ref_t, rows, cols)
        assert got.shape == (F, len(rows) - 1, len(cols) - 1, 5)
        np.testing.assert_array_equal(got, want, err_msg=f"{rows} {cols}")
        # the NULL index list: frames 0 .. n_sel - 1
        np.testing.assert_array_equal(_raw(dev, t, None, 2, ref_t, rows, cols), want[:2])
        # the sum over the tiling is kcmc_gradient_sums_u16's over its rectangle; one tile is that itself
        rect = (rows[0], rows[-1], cols[0], cols[-1])
        if rect[0] < rect[1] and rect[2] < rect[3]:
            five = _five(dev, t, [0, 1, 2], ref_t, rect)
            np.testing.assert_array_equal(got.sum(axis=(1, 2)), five)
            if got.shape[1:3] == (1, 1):
                np.testing.assert_array_equal(got[:, 0, 0], five)
        else:
            assert not got.any()


def test_wrapper_tiles_the_rectangle_over_one_slab_or_several(dev):
    H, W, rect, grid = 37, 61, (3, 34, 3, 58), (2, 3)
    x = _frames((F, H, W), 5)
    ref = _frames((H, W), 6)
    rows, cols = host.ref_tile_edges(H, W, grid, rect)
    idx = [2, 7, 0, 2, -1, 1, 3]  # a repeat, reversed order and indices outside the stack
    want = host.ref_tile_sums(x, idx, ref, rows, cols)
    assert not want[1].any() and not want[4].any() and not want[6].any() and want[0].any()
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    np.testing.assert_array_equal(_raw(dev, t, idx, len(idx), ref_t, rows, cols), want)
    got = refine_field.tile_gradient_sums(t, idx, ref_t, rect, grid)
    assert got.dtype == np.int64 and got.shape == (len(idx), 4, 6, 5)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(refine_field.tile_gradient_sums([t[:1].clone(), t[1:].clone()], idx, ref, rect, grid),
                                  want)
    assert refine_field.tile_gradient_sums(t, [], ref_t, rect, grid).shape == (0, 4, 6, 5)
    assert _raw(dev, t, [], 0, ref_t, rows, cols).shape == (0, 4, 6, 5)
    with pytest.raises(ValueError):
        refine_field.tile_gradient_sums(t, [0], ref_t, (0, 34, 3, 58), grid)
    # the frames' correlations from the tiles' totals are quality.frame_correlations'
    from kcmc_amd import quality

    gram = refine_field.tile_gram(ref, refine_field.tile_edges(H, W, grid, rect))
    np.testing.assert_array_equal(refine_field.correlations_from_tiles(got[[2, 5, 0]], gram),
                                  quality.frame_correlations(t, ref_t, rect))


def test_tile_sums_of_a_slab_that_starts_mid_allocation(dev):
    H, W = 40, 72
    rows, cols = (1, 7, 7, 19, 20, 39), (1, 5, 13, 14, 14, 37, 71)
    x = _frames((F, H, W), 5)
    ref = _frames((H, W), 6)
    want = host.ref_tile_sums(x, [0, 1, 2], ref, list(rows), list(cols))
    flat = torch.from_numpy(np.concatenate([np.zeros(4, np.uint16), x.ravel()])).to(dev)
    t = flat[4:].view(F, H, W)
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()  # W % 8 == 0, but the rows are off the 16-byte grid
    np.testing.assert_array_equal(_raw(dev, t, [0, 1, 2], F, torch.from_numpy(ref).to(dev), rows, cols), want)
    # ... and a misaligned reference beside aligned frames
    rflat = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), ref.ravel()])).to(dev)
    rt = rflat[1:].view(H, W)
    assert rt.data_ptr() % 16 == 2
    np.testing.assert_array_equal(_raw(dev, torch.from_numpy(x).to(dev), [0, 1, 2], F, rt, rows, cols), want)


@pytest.mark.parametrize("pattern", ["columns", "rows"])
def test_tile_sums_saturated(dev, pattern):
    """All-65535 frames against a reference of period 4 (0, 0, 65535, 65535) along the columns
    resp. the rows, in one 64 x 64 tile and in that tile with eight narrow ones around it: every gradient is +-65535 or
    0 and a 32-bit partial sum of a^2, a b or a g would wrap within two pixels."""
    H = W = 72
    line = np.array([0, 0, 65535, 65535], np.uint16)
    ref = np.tile(line, (H, W // 4))[:, :W] if pattern == "columns" else np.tile(line[:, None], (H // 4, W))[:H]
    ref = np.ascontiguousarray(ref)
    x = np.full((F, H, W), 65535, np.uint16)
    t, ref_t = torch.from_numpy(x).to(dev), torch.from_numpy(ref).to(dev)
    for rows, cols in (((4, 68), (4, 68)), ((1, 4, 68, 71), (1, 4, 68, 71))):
        want = host.ref_tile_sums(x, [0, 1, 2], ref, list(rows), list(cols))
        mid = want[0, len(rows) // 2 - 1, len(cols) // 2 - 1]
        assert mid[1] == 64 * 64 * 65535 ** 2 and mid[2] == 32 * 64 * 65535 ** 2
        np.testing.assert_array_equal(_raw(dev, t, [0, 1, 2], F, ref_t, rows, cols), want)


def test_entry_point_validation(dev):
    H, W = 33, 40
    fr = torch.zeros((1, H, W), dtype=torch.int16, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = torch.zeros((H, W), dtype=torch.int16, device=dev)
    out = torch.zeros((2, 3, 5), dtype=torch.int64, device=dev)
    host.check_validation(_ctx(dev).handle, (fr.data_ptr(), idx.data_ptr(), ref.data_ptr(), out.data_ptr()))


# --------------------------------------------------------------------------- end to end
# host.e2e_stack(): test_gpu_refine.py's kind of stack with a smooth field added to every
# frame's motion; tests/test_refine_field_host.py checks on the CPU that the restatement alone
# steps every node of every frame and keeps every frame in the first iteration.
GRID = host.GRID


def _va(devices=(0,), **kw):
    return type("VA", (VideoAligner,), {"DEVICES": list(devices), "REFINE": "intensity", **kw})()


def _run(va):
    e = host.e2e_stack()
    return va.align_keypoints(e["frames"], e["kp_tpl"], e["des_tpl"], e["kq"], e["dq"], n_kp_global=40)


@pytest.fixture(scope="module")
def e2e(dev):
    """Every end-to-end run, made once."""
    out = {}
    for name, va in (("parent", _va()), ("off", _va(REFINE_GRID=None)), ("on", _va(REFINE_GRID=GRID)),
                     ("on2", _va((0, 0), REFINE_GRID=GRID)), ("two", _va(REFINE_GRID=GRID, REFINE_GRID_ITERS=2))):
        out[name] = (va, _run(va))
    return out


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert list(a[2]) == list(b[2])


def test_grid_off_changes_nothing(e2e):
    _same(e2e["off"][1], e2e["parent"][1])
    for name in ("parent", "off"):
        va = e2e[name][0]
        for attr in ("refine_field", "refine_field_correlations", "refine_field_idxs"):
            assert getattr(va, attr) is None, (name, attr)
        assert va.refine_steps is not None
    np.testing.assert_array_equal(e2e["off"][0].affines, e2e["parent"][0].affines)
    np.testing.assert_array_equal(e2e["off"][0].refine_steps, e2e["parent"][0].refine_steps)
    aligned, _, skipped = e2e["off"][1]
    assert list(skipped) == []  # the premise: every frame has a model
    e = host.e2e_stack()
    for f in range(host.EF):  # the refinement's frames: the affine warp of their sources
        np.testing.assert_array_equal(aligned[f], oracle.warp_affine_u16(e["frames"][f], e2e["off"][0].affines[f]))


def _check_against_restatement(va, result, off, iters):
    e = host.e2e_stack()
    va0, (off_aligned, off_eu, skipped) = off
    aligned, eu, skipped2 = result
    w_aligned, w_field, w_corr, w_idxs, w_steps = host.ref_field_pass(off_aligned, e["frames"], va0.affines[:host.EF],
                                                                      skipped, GRID, iters=iters)
    assert va.refine_field.shape == (host.EF, *GRID, 2) and va.refine_field.dtype == np.float64
    assert va.refine_field_correlations.shape == (host.EF, iters + 1)
    np.testing.assert_array_equal(va.refine_field, w_field)
    np.testing.assert_array_equal(va.refine_field_correlations, w_corr)
    assert va.refine_field_idxs == w_idxs
    np.testing.assert_array_equal(aligned, w_aligned)
    # the maps, the transform summary and the lists are the run's without the grid
    np.testing.assert_array_equal(va.affines, va0.affines)
    np.testing.assert_array_equal(eu, off_eu)
    assert list(skipped2) == list(skipped) and va.interpolated_idxs == va0.interpolated_idxs
    np.testing.assert_array_equal(va.refine_steps, va0.refine_steps)
    return w_steps


def test_field_run_equals_the_host_restatement_and_lowers_the_error(e2e):
    e = host.e2e_stack()
    va, res = e2e["on"]
    steps = _check_against_restatement(va, res, e2e["off"], 1)
    c = va.refine_field_correlations
    # nothing passes by rejecting everything: every node of every frame stepped, every frame was kept
    host.check_first_iteration(steps, c, va.refine_field_idxs, host.EF)
    np.testing.assert_array_equal(va.refine_field, steps[0])
    assert (c[:, 1] >= c[:, 0]).all() and (c[:, 1] > c[:, 0]).any()
    zero = host.node_errors(np.zeros_like(e["fields"]), e["fields"])
    err = host.node_errors(va.refine_field, e["fields"])
    rms = lambda v: float(np.sqrt((v ** 2).mean()))  # noqa: E731
    print("RMS node error", rms(zero), "->", rms(err), "mean r", c[:, 0].mean(), "->", c[:, 1].mean())
    assert rms(err) < rms(zero)
    # two slabs on one GPU equal one slab
    va2, res2 = e2e["on2"]
    _same(res2, res)
    np.testing.assert_array_equal(va2.refine_field, va.refine_field)
    np.testing.assert_array_equal(va2.refine_field_correlations, va.refine_field_correlations)
    assert va2.refine_field_idxs == va.refine_field_idxs


def test_two_field_iterations_equal_the_host_restatement(e2e):
    va, res = e2e["two"]
    _check_against_restatement(va, res, e2e["off"], 2)
    c = va.refine_field_correlations
    assert (c[:, 2] >= c[:, 1]).all()  # columns 1 and 2 share the last iteration's reference image
