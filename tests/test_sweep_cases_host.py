"""What the committed seeds of tests/sweep_cases.py reach (no GPU): every assertion runs over the
seeds of one generator and names a path of the kernel the sweep is there for.  When one fails,
the seed list or the generator's forcing rules change, not the assertion.  And the restatements
the sweeps compare with agree with each other where their definitions overlap."""
import numpy as np
import pytest

import oracle
import sweep_cases as sc
import test_fallback_host as fhost
import test_normalize_host as nhost
import test_piecewise_host as phost
import test_quality_host as qhost
import test_refine_field_host as tfhost
import test_refine_host as rhost
import test_warp_linear_host as wl


@pytest.fixture(scope="module")
def cases():
    return {k: [sc.GENERATORS[k](s) for s in sc.SEEDS[k]] for k in sc.KERNELS}


def test_sixteen_seeds_per_kernel_and_reproducible_cases():
    for k in sc.KERNELS:
        assert len(sc.SEEDS[k]) == 16 and len(set(sc.SEEDS[k])) == 16
        a, b = sc.GENERATORS[k](sc.SEEDS[k][1]), sc.GENERATORS[k](sc.SEEDS[k][1])
        assert sc.describe(a) == sc.describe(b) and np.array_equal(a["frames"], b["frames"])
    for k, s in sc.PINNED:
        assert k in sc.KERNELS and s not in sc.SEEDS[k]


def _tile_columns(c):  # csrc/shift_search.hip: tiles of 64 columns from the 8-aligned left edge
    _, _, x0, x1 = c["rect"]
    return (x1 - (x0 & ~7) + 63) // 64


def _staging_of_called(c):
    vec = sc.vector_slabs(c)
    return {vec[i] for i in sc.called_slabs(c)}


def test_shift_search_seeds(cases):
    cs = cases["shift_search"]
    R = [c["R"] for c in cs]
    assert all(1 <= r <= 16 for r in R)
    # (2R + 1)^2 shifts over at most 512 threads: one, two and three per thread
    assert any(r <= 10 for r in R) and any(11 <= r <= 15 for r in R) and any(r == 16 for r in R)
    assert any(_tile_columns(c) >= 3 for c in cs)
    assert any(c["rect"][1] - c["rect"][0] == 1 and c["rect"][3] - c["rect"][2] == 1 for c in cs)
    w8 = [c for c in cs if c["W"] % 8 == 0]
    assert any(True in _staging_of_called(c) for c in w8)
    assert any(False in _staging_of_called(c) for c in w8)
    assert any(any(not 0 <= f < c["F"] for f in c["idx"]) for c in cs)
    for c in cs:
        y0, y1, x0, x1 = c["rect"]
        assert c["R"] <= y0 < y1 <= c["H"] - c["R"] and c["R"] <= x0 < x1 <= c["W"] - c["R"]


def test_gradient_sums_seeds(cases):
    cs = cases["gradient_sums"]
    assert any(c["rows"] is None for c in cs) and any(c["rows"] is not None for c in cs)
    assert any(c["rect"] == (1, c["H"] - 1, 1, c["W"] - 1) for c in cs)
    for c in cs:
        y0, y1, x0, x1 = c["rect"]
        assert 1 <= y0 < y1 <= c["H"] - 1 and 1 <= x0 < x1 <= c["W"] - 1


def thread_columns_log2(nvec):
    """csrc/u16_rows.h: the largest power of two in [8, 256] that idles at most 1/8 of the thread
    columns over a row of nvec vectors, else the one that idles fewest (the larger on a tie)."""
    best, best_l = None, 3
    for l in range(8, 2, -1):
        used = -(-nvec // (1 << l)) << l
        if used * 8 <= nvec * 9:
            return l
        if best is None or used < best:
            best, best_l = used, l
    return best_l


def test_thread_columns_rule():
    assert [thread_columns_log2(n) for n in (1, 8, 9, 16, 32, 41, 64, 258, 256)] == [3, 3, 4, 4, 5, 4, 6, 5, 8]


def test_tile_gradient_sums_seeds(cases):
    cs = cases["tile_gradient_sums"]
    assert any(32 in (len(c["row_edges"]) - 1, len(c["col_edges"]) - 1) for c in cs)
    inner_empty = lambda e: any(a == b for a, b in zip(e[:-1], e[1:]))  # noqa: E731
    assert any(inner_empty(c["col_edges"]) for c in cs) and any(inner_empty(c["row_edges"]) for c in cs)
    assert any(1 in np.diff(c["col_edges"]) for c in cs)
    classes = set()
    for c in cs:
        x0, x1 = c["col_edges"][0], c["col_edges"][-1]
        if x0 < x1 and c["row_edges"][0] < c["row_edges"][-1]:
            classes.add(thread_columns_log2((x1 + 7) // 8 - x0 // 8))
    assert len(classes) >= 4, classes
    assert {True, False} <= set().union(*(_staging_of_called(c) for c in cs))
    for c in cs:
        for e, L in ((c["row_edges"], c["H"]), (c["col_edges"], c["W"])):
            assert 2 <= len(e) <= 33 and (np.diff(e) >= 0).all() and 1 <= e[0] and e[-1] <= L - 1


def test_phase_sums_seeds(cases):
    cs = cases["phase_sums"]
    assert any(c["R"] == 0 for c in cs) and any(c["R"] == 16 for c in cs)
    assert any(c["W"] == 2 * c["R"] + 1 for c in cs)
    assert any(c["W"] < 4 * c["R"] for c in cs)
    assert any(c["W"] > 1024 for c in cs)
    assert any(c["H"] % 2 for c in cs) and any(c["H"] % 2 == 0 for c in cs)
    assert all(c["H"] >= 2 and c["W"] >= 2 * c["R"] + 1 for c in cs)


def test_warp_field_seeds(cases):
    cs = cases["warp_field"]
    assert {c["family"] for c in cs} == set(sc.FIELD_FAMILIES)
    assert any(c["W"] < 128 for c in cs) and any(c["H"] < 56 for c in cs)
    assert any(c["gy"] == c["H"] or c["gx"] == c["W"] for c in cs)
    assert any(c["H"] % 64 == 0 and c["H"] % 56 != 0 for c in cs)
    assert any(np.isnan(c["M"]).any() for c in cs)
    assert {c["inverse_map"] for c in cs} == {False, True}
    assert any(c["W"] % 2 for c in cs)
    for c in cs:
        assert 1 <= c["gy"] <= min(16, c["H"]) and 1 <= c["gx"] <= min(16, c["W"])
        assert np.abs(c["q"]).max() <= 1 << 20  # the contract; the far node sits on its edge
        assert (np.abs(c["q"]) == 1 << 20).sum() == (c["family"] == "2px+far")


def test_resize_seeds(cases):
    cs = cases["resize_u8"]
    assert any(c["dst_h"] > c["H"] for c in cs) and any(c["dst_h"] < c["H"] for c in cs)
    assert any(c["dst_w"] > c["W"] for c in cs) and any(c["dst_w"] < c["W"] for c in cs)
    assert any(1 in (c["H"], c["W"], c["dst_h"], c["dst_w"]) for c in cs)
    assert any(c["dst_h"] == c["H"] or c["dst_w"] == c["W"] for c in cs)
    assert all(1 <= v <= 400 for c in cs for v in (c["H"], c["W"], c["dst_h"], c["dst_w"]))


def test_normalize_seeds(cases):
    """What only this sweep puts in front of stages.brightest_px: part lists with copied parts
    and every tail length, and percentiles whose two ranks (test_normalize_host.ranks) sit in
    different coarse bins, on both branches of numpy's interpolation."""
    cs = cases["normalize"]
    split, gammas = 0, []
    for c in cs:
        s = np.sort(c["frames"].reshape(-1))
        lo, hi, gamma = nhost.ranks(s.size, c["percentile"])
        if s[lo] >> 8 != s[hi] >> 8:  # a fine pass per rank
            split += 1
            gammas.append(gamma)
    assert split >= 1
    assert any(g >= 0.5 for g in gammas) and any(0 < g < 0.5 for g in gammas)  # among the split ones
    all_g = [nhost.ranks(c["frames"].size, c["percentile"])[2] for c in cs]
    assert any(g >= 0.5 for g in all_g) and any(g < 0.5 for g in all_g)
    parts = [((b - a) * c["H"] * c["W"], off) for c in cs for a, b, off in c["slabs"]]
    assert any(off % 8 for _, off in parts)  # not on the 16-byte grid: stages._aligned16 copies it
    assert {n % 8 for n, _ in parts} == set(range(8))
    assert any(isinstance(sc._parts(c, "cpu"), list) for c in cs)  # handed over as a part list
    # the draws of the generator's docstring
    assert {c["family"] for c in cs} == {"shared", "concentrated"}
    assert {c["max_px"] for c in cs} == {255, 127}
    assert set(sc.NORMALIZE_Q) <= {c["percentile"] for c in cs}
    assert any(c["percentile"] not in sc.NORMALIZE_Q for c in cs)
    assert all(1 <= c["F"] <= 6 and 1 <= c["H"] <= 300 and 1 <= c["W"] <= 300 for c in cs)
    assert all(0.0 <= c["percentile"] <= 100.0 for c in cs)


def test_normalize_expected_is_numpys_and_compare_is_sensitive():
    c = next(c for c in map(sc.case_normalize, sc.SEEDS["normalize"]) if c["frames"].size > 1000)
    want = sc.expected("normalize", c)
    assert want["brightest"] == np.percentile(c["frames"], c["percentile"])
    assert want["out"].dtype == np.uint8 and want["out"].shape == c["frames"].shape
    sc.compare("normalize", c, {"brightest": want["brightest"], "out": want["out"].copy(), "guards": True}, want)
    wrong = want["out"].copy()
    wrong.reshape(-1)[-1] ^= 1
    for got in ({"brightest": want["brightest"], "out": wrong, "guards": True},
                {"brightest": np.nextafter(want["brightest"], np.inf), "out": want["out"], "guards": True},
                {"brightest": want["brightest"], "out": want["out"], "guards": False}):
        with pytest.raises(AssertionError):
            sc.compare("normalize", c, got, want)
    assert sc.scale_divisor(np.float64(0.0)) == 1.0 and sc.scale_divisor(np.float64(3.5)) == 3.5


# ------------------------------------------------------------------ the bilinear warps
# What the two sweeps are for: csrc/warp.hip decides its 16-byte staging loads, its buffer loads
# and stores and its 4-byte pixel-pair stores from W alone, never from the pointers, so the seeds
# must put every such access on and off its grid.  test_warp_linear_host restates both plan
# kernels and names the tile kernels' paths; here every frame's paths are crossed with the
# offsets of the slab that holds it.
LINEAR = {"warp_affine": (wl.affine_paths, wl.AFFINE_PATHS), "warp_perspective": (wl.persp_paths, wl.PERSP_PATHS)}
SRC_PHASES = {0: "on the grid", 8: "on the grid", 1: "2 bytes off", 4: "8 bytes off"}  # of 16 bytes, per OFFS_U16


def linear_reach(kernel, cs):
    """(paths, src, dst) of the frames of ``cs``.  paths: the union of the tile kernel's paths.
    src: (group, mode, phase of the source slab on the 16-byte grid) of every vector-staged frame
    -- W % 8 == 0 and a tile on mode 3 or mode 0; group vec1 / vecC by the channels.  dst: (kind,
    output offset odd) of every dword-stored frame -- kind "pairs": C = 1, W even and a tile on
    mode 0, 1 or 2 (a pixel pair as one dword); "channels": C = 3 or 4 and W >= 2 (two pixels as C
    dwords; a frame whose map holds a NaN is stored by mode 1 like any other); "fast": a mode-3
    tile (one b32 / b96 / b128 buffer store per lane)."""
    paths_of = LINEAR[kernel][0]
    paths, src, dst = set(), set(), set()
    for c in cs:
        for f in range(c["F"]):
            p = paths_of(c["frames"][f], c["M"][f], c["inverse_map"])
            off, o_off = sc.frame_slab(c, f)
            paths |= set(p)
            nan = "nan" in p  # every tile of the frame is on mode 1, whatever the restatement counted
            for mode in ("mode3", "mode0"):
                if c["W"] % 8 == 0 and mode in p and not nan:
                    src.add(("vec1" if c["C"] == 1 else "vecC", mode, SRC_PHASES[off]))
            if c["C"] == 1 and c["W"] % 2 == 0 and (nan or {"mode0", "mode1", "mode2"} & set(p)):
                dst.add(("pairs", o_off % 2))
            if c["C"] > 1 and c["W"] >= 2:
                dst.add(("channels", o_off % 2))
            if "mode3" in p and not nan:
                dst |= {("fast", o_off % 2), (f"fast-C{c['C']}", o_off % 2)}  # the latter: b32, b96, b128
    return paths, src, dst


def linear_demands(kernel):
    """What linear_reach of the committed seeds must hold: every path; each group of vector-staged
    frames at each phase of the source, for the affine kernel on mode 3 and on mode 0 separately;
    each kind of dword-stored frame at an even and at an odd output offset.  The perspective
    kernel has no mode 3, hence neither that staging nor the "fast" stores."""
    modes = ("mode3", "mode0") if kernel == "warp_affine" else ("mode0",)
    kinds = ("pairs", "channels")
    if kernel == "warp_affine":
        kinds += ("fast", "fast-C1", "fast-C3", "fast-C4")  # and each width of the fast store by itself
    src = {(g, m, ph) for g in ("vec1", "vecC") for m in modes for ph in set(SRC_PHASES.values())}
    return LINEAR[kernel][1], src, {(k, odd) for k in kinds for odd in (0, 1)}


@pytest.mark.parametrize("kernel", sorted(LINEAR))
def test_linear_warp_seeds(cases, kernel):
    cs = cases[kernel]
    paths, src, dst = linear_reach(kernel, cs)
    want_paths, want_src, want_dst = linear_demands(kernel)
    assert paths == want_paths, (want_paths - paths, paths - want_paths)
    assert src >= want_src, sorted(want_src - src)
    assert dst >= want_dst, sorted(want_dst - dst)
    # the draws of the generator's docstring
    assert all(1 <= c["F"] <= 3 and 1 <= c["H"] <= 130 and 1 <= c["W"] <= 300 for c in cs)
    assert all(c["C"] == (1, 1, 3, 4)[s % 4] for s, c in zip(sc.SEEDS[kernel], cs))
    assert sum(c["W"] % 8 == 0 for c in cs) >= 8 and any(c["W"] % 2 for c in cs)
    assert {c["C"] for c in cs if c["W"] % 8 == 0} == {1, 3, 4}  # the b32, b96 and b128 stores of mode 3
    assert {fam for c in cs for fam in c["families"]} == set(sc.LINEAR_FAMILIES)
    assert {c["inverse_map"] for c in cs} == {False, True}
    assert any(np.isnan(c["M"][-1]).any() for c in cs) and not any(np.isnan(c["M"][:-1]).any() for c in cs)
    assert any(-(-c["W"] // 128) == 3 for c in cs)  # three tile columns
    # a tile is 128 x 56 (x 64) with one channel and 128 x 24 with more: a case is small
    assert all(c["frames"].size <= 3 * 130 * 300 * 4 for c in cs)


def test_linear_warp_sources_are_guarded_and_compare_is_sensitive():
    """Without a device: the source views sit between nonzero fills inside their allocations, and
    compare refuses an output that is off by one in one pixel, and one whose sentinels are gone."""
    import torch

    cpu = torch.device("cpu")
    arr = np.arange(1, 25, dtype=np.uint16).reshape(2, 3, 4)
    for off in sc.OFFS_U16:
        v = sc._view(arr, off, cpu, sc.GUARD_U16, sc._GUARD)
        flat = torch.as_strided(v, (off + arr.size + sc._GUARD,), (1,), v.storage_offset() - off).numpy()
        assert v.is_contiguous() and v.storage_offset() == off and np.array_equal(v.numpy(), arr)
        assert (flat[:off] == sc.GUARD_U16).all() and (flat[off + arr.size:] == sc.GUARD_U16).all()
        assert len(flat[off + arr.size:]) >= 64
    z = sc._view(arr, 4, cpu)  # the other kernels' views: zeros in front, nothing behind
    assert z.storage_offset() == 4 and z.untyped_storage().nbytes() == 2 * (4 + arr.size)
    for kernel in sorted(LINEAR):
        c = next(c for c in map(sc.GENERATORS[kernel], sc.SEEDS[kernel]) if c["frames"].size > 1000)
        want = sc.expected(kernel, c)
        assert want["out"].shape == c["frames"].shape and want["out"].dtype == np.uint16
        sc.compare(kernel, c, {"out": want["out"].copy(), "guards": True}, want)
        wrong = want["out"].copy()
        wrong.reshape(-1)[wrong.size // 2] ^= 1  # one pixel, by one
        with pytest.raises(AssertionError):
            sc.compare(kernel, c, {"out": wrong, "guards": True}, want)
        with pytest.raises(AssertionError):
            sc.compare(kernel, c, {"out": want["out"].copy(), "guards": False}, want)


@pytest.mark.parametrize("kernel", sc.KERNELS)
def test_every_generator_draws_every_offset_and_three_slabs(cases, kernel):
    cs = cases[kernel]
    offs = sc.OFFS_U8 if kernel == "resize_u8" else sc.OFFS_U16
    assert {off for c in cs for _, _, off in c["slabs"]} == set(offs)
    assert any(len(c["slabs"]) == 3 for c in cs)
    for c in cs:
        assert c["slabs"][0][0] == 0 and c["slabs"][-1][1] == c["F"]
        assert all(a < b for a, b, _ in c["slabs"])
        assert all(p[1] == n[0] for p, n in zip(c["slabs"], c["slabs"][1:]))
    if "ref_off" in cs[0]:
        assert {c["ref_off"] for c in cs} == set(offs)
    if "out_offs" in cs[0]:
        assert {o for c in cs for o in c["out_offs"]} == set(offs)
    if "idx" in cs[0]:
        assert any(c["idx"] == list(range(c["F"])) for c in cs) and any(len(c["idx"]) == 0 for c in cs)
        assert any(-1 in c["idx"] for c in cs) and any(max(c["idx"], default=0) >= c["F"] for c in cs)
        assert any(len(set(c["idx"])) < len(c["idx"]) for c in cs)
        assert any(any(a > b >= 0 for a, b in zip(c["idx"], c["idx"][1:])) for c in cs)


def test_expected_lays_the_frames_out_over_the_index_list():
    c = sc.case_tile_gradient_sums(1)
    c["idx"] = [c["F"], 0, -1, 0, c["F"] - 1]
    want = tfhost.ref_tile_sums(c["frames"], c["idx"], c["ref"], c["row_edges"], c["col_edges"])
    np.testing.assert_array_equal(sc.expected("tile_gradient_sums", c)["sums"], want)
    assert not want[0].any() and not want[2].any()


# ------------------------------------------------------------------ the restatements agree
def test_shift_search_restatement_at_zero_shift_is_frame_stats():
    c = sc.case_shift_search(1)
    R, idx = c["R"], list(range(c["F"]))
    got = fhost.ref_shift_search(c["frames"], idx, c["ref"], c["rect"], R)
    np.testing.assert_array_equal(got[:, R, R], qhost.ref_frame_stats(c["frames"], c["ref"], c["rect"]))


def test_tile_restatement_sums_to_the_gradient_sums_restatement():
    c = next(c for c in map(sc.case_tile_gradient_sums, range(16))
             if c["row_edges"][0] < c["row_edges"][-1] and c["col_edges"][0] < c["col_edges"][-1])
    idx = list(range(c["F"]))
    rect = (c["row_edges"][0], c["row_edges"][-1], c["col_edges"][0], c["col_edges"][-1])
    tiles = tfhost.ref_tile_sums(c["frames"], idx, c["ref"], c["row_edges"], c["col_edges"])
    whole = rhost.ref_gradient_sums(c["frames"], idx, c["ref"], rect)
    np.testing.assert_array_equal(tiles.sum(axis=(1, 2)), whole[:, :5].astype(np.int64))


def test_field_restatement_with_a_zero_field_is_the_oracle_warp():
    c = next(c for c in map(sc.case_warp_field, range(16)) if c["family"] != "zero" and c["H"] * c["W"] > 1000)
    q = np.zeros_like(c["q"])
    got = phost.ref_warp_field(c["frames"], c["M"], q, (c["gy"], c["gx"]), c["inverse_map"])
    for f in range(c["F"]):
        np.testing.assert_array_equal(got[f], oracle.warp_affine_u16(c["frames"][f], c["M"][f],
                                                                     inverse_map=c["inverse_map"]))
