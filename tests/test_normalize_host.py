"""The index arithmetic of csrc/normalize.hip restated (no GPU): which threads of the two
histogram passes and of the table kernel take which path at a given stack size, from the
constants in the kernel's own text.  hist256_u16_kernel and lut_u16_to_u8_kernel are the only
kernels that cap their grid and walk the rest with a grid-stride loop; below the cap the
histogram's main loop never runs, so a test reaches it only with a stack chosen for it.  The
sizes of tests/test_gpu_normalize.py are defined here, each with an assertion of the path it is
named for, and so is numpy's choice of the two ranks of a percentile (ranks), which the directed
cases there and the sweep's reach assertions (tests/test_sweep_cases_host.py) use.

A change of a cap or of the block size fails test_constants_in_the_kernel_text; the sizes then
have to be chosen again, not the assertions."""
import os
import re

import numpy as np
import pytest

from kcmc_amd import build as kbuild
from kcmc_amd import stages

with open(os.path.join(kbuild.CSRC, "normalize.hip")) as _f:
    _TEXT = _f.read()


def _const(pattern):
    m = re.findall(pattern, _TEXT)
    assert len(m) == 1, (pattern, m)
    return int(m[0])


THREADS = _const(r"constexpr\s+int\s+kThreads\s*=\s*(\d+)\s*;")
CAP_COARSE = _const(r"hist256_u16_kernel<64>\s*,\s*dim3\(grid_for\(n / 8 \+ 1,\s*(\d+)\)\)")
CAP_FINE = _const(r"hist256_u16_kernel<8>\s*,\s*dim3\(grid_for\(n / 8 \+ 1,\s*(\d+)\)\)")
CAP_TABLE = _const(r"int\s+grid_for\(size_t\s+work_items,\s*size_t\s+cap\s*=\s*(\d+)\)")

SIZE_A = 8 * (3 * 1048576 + 777) + 5
SIZE_B = 16 * (2 * 1048576 + 333) + 13
EDGE_NO_LOOP = 4194311
EDGE_ONE_LOOP = 4194312
LARGEST_BEFORE = 2 * 1080 * 1920  # test_gpu_models.test_brightest_px_matches_numpy
LARGE_SIZES = (SIZE_A, SIZE_B, EDGE_ONE_LOOP)


def test_constants_in_the_kernel_text():
    assert (THREADS, CAP_COARSE, CAP_FINE, CAP_TABLE) == (256, 2048, 4096, 4096)
    # the launches the patterns above did not pin: 256 threads, the table kernel on the default cap
    assert len(re.findall(r"dim3\(kThreads\)", _TEXT)) == 3
    assert len(re.findall(r"lut_u16_to_u8_kernel,\s*dim3\(grid_for\(n / 16 \+ 1\)\)", _TEXT)) == 1
    assert "for (; i + stride < n8; i += 2 * stride)" in _TEXT
    assert "i < n16; i += stride)" in _TEXT


# ------------------------------------------------------------------ the model
def grid_for(work_items, cap, threads=None):
    threads = THREADS if threads is None else threads
    return max(1, min(-(-work_items // threads), cap))


def hist_paths(n, cap, threads=None):
    """hist256_u16_kernel over n values on grid_for(n / 8 + 1, cap) blocks.  Per thread (indexed by
    its first vector i0 = blockIdx.x * kThreads + tid): ``iters`` main-loop iterations (two loads
    each), ``single`` whether the load after the loop runs; ``tail`` the n % 8 values of block 0."""
    threads = THREADS if threads is None else threads
    n8 = n // 8
    grid = grid_for(n8 + 1, cap, threads)
    stride = grid * threads
    i0 = np.arange(stride, dtype=np.int64)
    # iterations k = 0, 1, ... while i0 + 2 k stride + stride < n8
    iters = np.maximum(0, -(-(n8 - i0 - stride) // (2 * stride)))
    single = i0 + 2 * iters * stride < n8
    # thread i0 loads i0 + m stride for m < 2 iters + single: each vector below n8 exactly once
    assert np.array_equal(2 * iters + single, np.maximum(0, -(-(n8 - i0) // stride)))
    return {"grid": grid, "stride": stride, "iters": iters, "single": single, "tail": n - 8 * n8}


def table_paths(n, cap=None, threads=None):
    """lut_u16_to_u8_kernel: ``iters`` steps of 16 values per thread, ``tail`` n % 16."""
    threads = THREADS if threads is None else threads
    n16 = n // 16
    grid = grid_for(n16 + 1, CAP_TABLE if cap is None else cap, threads)
    stride = grid * threads
    i0 = np.arange(stride, dtype=np.int64)
    return {"grid": grid, "stride": stride, "iters": np.maximum(0, -(-(n16 - i0) // stride)), "tail": n - 16 * n16}


def _walk_hist(n8, stride, i0):
    """One thread of the histogram kernel, statement by statement: the vectors it loads."""
    got, i = [], i0
    while i + stride < n8:
        got += [i, i + stride]
        i += 2 * stride
    if i < n8:
        got.append(i)
    return got


def test_model_equals_the_loop_walked_literally():
    """With a small block and cap (4 threads, 3 blocks) so that every n up to some hundred runs
    through capped and uncapped grids: the closed forms of hist_paths / table_paths equal the
    kernel's loops walked one statement at a time, and the loads cover [0, n / 8) once."""
    for n in range(0, 700):
        p = hist_paths(n, 3, 4)
        seen = []
        for i0 in range(p["stride"]):
            w = _walk_hist(n // 8, p["stride"], i0)
            assert len(w) == 2 * p["iters"][i0] + p["single"][i0]
            assert (len(w) % 2 == 1) == bool(p["single"][i0])
            seen += w
        assert sorted(seen) == list(range(n // 8)) and p["tail"] == n % 8
        t = table_paths(n, 3, 4)
        steps = [len(range(i0, n // 16, t["stride"])) for i0 in range(t["stride"])]
        assert steps == t["iters"].tolist() and sum(steps) == n // 16 and t["tail"] == n % 16
    assert hist_paths(8 * 12 - 1, 3, 4)["iters"].max() == 0 and hist_paths(8 * 13, 3, 4)["iters"].max() == 1


# ------------------------------------------------------------------ the sizes of the GPU tests
def test_size_a():
    c, f, t = hist_paths(SIZE_A, CAP_COARSE), hist_paths(SIZE_A, CAP_FINE), table_paths(SIZE_A)
    assert SIZE_A == 25172045 and c["grid"] == CAP_COARSE and f["grid"] == CAP_FINE and t["grid"] == CAP_TABLE
    assert (c["iters"] == 3).all() and int(c["single"].sum()) == 777 and c["tail"] == 5
    assert int((f["iters"] == 2).sum()) == 777 and not f["single"][f["iters"] == 2].any()
    assert (f["iters"][~(f["iters"] == 2)] == 1).all() and f["single"][f["iters"] == 1].all() and f["tail"] == 5
    assert t["iters"].max() == 2 and t["iters"].min() == 1 and t["tail"] == 13


def test_size_b():
    c, f, t = hist_paths(SIZE_B, CAP_COARSE), hist_paths(SIZE_B, CAP_FINE), table_paths(SIZE_B)
    assert SIZE_B == 33559773
    assert t["iters"].max() == 3 and int((t["iters"] == 3).sum()) == 333 and t["iters"].min() == 2 and t["tail"] == 13
    assert (c["iters"] == 4).all() and c["single"].any() and not c["single"].all() and c["tail"] == 5
    assert (f["iters"] == 2).all() and f["single"].any()


def test_loop_edges():
    for cap in (CAP_COARSE, CAP_FINE):
        first = 8 * cap * THREADS + 8  # n / 8 == stride + 1: thread 0 loads vectors 0 and stride
        below, at = hist_paths(first - 1, cap), hist_paths(first, cap)
        assert below["grid"] == at["grid"] == cap
        assert below["iters"].max() == 0 and below["single"].all() and below["tail"] == 7
        assert at["iters"].tolist()[:2] == [1, 0] and int(at["iters"].sum()) == 1
        assert not at["single"][0] and at["single"][1:].all() and at["tail"] == 0
    assert (EDGE_NO_LOOP, EDGE_ONE_LOOP) == (8 * CAP_COARSE * THREADS + 7, 8 * CAP_COARSE * THREADS + 8)
    assert 8 * CAP_FINE * THREADS + 8 == 8388616
    # the fine pass and the table kernel at the coarse edge: still one load, one step
    assert hist_paths(EDGE_ONE_LOOP, CAP_FINE)["iters"].max() == 0
    assert table_paths(EDGE_ONE_LOOP)["iters"].max() == 1
    first16 = 16 * CAP_TABLE * THREADS + 16
    assert first16 == 16777232
    assert table_paths(first16 - 1)["iters"].max() == 1 and table_paths(first16)["iters"].tolist()[:2] == [2, 1]


def test_the_largest_stack_of_the_other_tests_reaches_no_loop():
    """Why the sizes above exist: 2 x 1080 x 1920, the largest stack test_gpu_models,
    test_gpu_fuzz and test_gpu_multidevice hand to brightest_px, stays below every cap."""
    c, f, t = (hist_paths(LARGEST_BEFORE, CAP_COARSE), hist_paths(LARGEST_BEFORE, CAP_FINE),
               table_paths(LARGEST_BEFORE))
    assert c["grid"] == 2026 < CAP_COARSE and f["grid"] == 2026 and t["grid"] == 1013
    assert c["iters"].max() == 0 and f["iters"].max() == 0 and t["iters"].max() == 1
    assert c["tail"] == 0 and t["tail"] == 0


def test_the_large_sizes_together_reach_every_path():
    hist = [hist_paths(n, cap) for n in LARGE_SIZES for cap in (CAP_COARSE, CAP_FINE)]
    for cap in (CAP_COARSE, CAP_FINE):  # two or more iterations, and the single load behind one
        ps = [hist_paths(n, cap) for n in LARGE_SIZES]
        assert any(p["iters"].max() >= 2 for p in ps)
        assert any((p["single"] & (p["iters"] >= 1)).any() for p in ps)
        assert any((~p["single"] & (p["iters"] >= 1)).any() for p in ps)
    assert all(p["tail"] for p in hist[:4]) and all(table_paths(n)["tail"] for n in LARGE_SIZES[:2])
    assert {int(table_paths(n)["iters"].max()) for n in LARGE_SIZES} == {1, 2, 3}
    assert all(n < 2 ** 32 for n in LARGE_SIZES)


# ------------------------------------------------------------------ numpy's two ranks
def ranks(n, q):
    """(lo, hi, gamma) of np.percentile(a, q) over n elements ('linear'): the two order statistics
    it reads and the weight of the upper one."""
    vi = (n - 1) * np.true_divide(np.float64(q), 100)
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    lo = int(np.floor(vi))
    return lo, lo + 1, float(vi - lo)


def q_for_rank(n, k, frac):
    """A q whose floor rank is k and whose gamma is about frac (0 < frac < 1)."""
    q = 100.0 * (k + frac) / (n - 1)
    lo, hi, gamma = ranks(n, q)
    assert (lo, hi) == (k, k + 1) and abs(gamma - frac) < 1e-6
    return q


def test_ranks_restates_numpy():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 300))
        s = np.sort(rng.integers(0, 65536, n)).astype(np.float64) * 3.0  # distinct enough to expose a wrong rank
        q = float(rng.choice([0.0, 100.0, 99.99, rng.uniform(0, 100)]))
        lo, hi, g = ranks(n, q)
        assert np.percentile(s, q) == pytest.approx(s[lo] + (s[hi] - s[lo]) * g, rel=1e-12)
    assert ranks(1, 37.0) == (0, 0, 0.0) and ranks(2, 0.0) == (0, 1, 0.0)


# ------------------------------------------------------------------ the table
SCALE_B = (1234.567, 0.5, 65535.0, 4095.0)
SCALE_MAX_PX = (255, 127, 200)


@pytest.mark.parametrize("max_px", SCALE_MAX_PX)
@pytest.mark.parametrize("b", SCALE_B)
def test_max_scale_lut_is_the_expression_over_every_value(b, max_px):
    v = np.arange(65536, dtype=np.uint16)
    want = np.clip(v / b * max_px, a_min=0, a_max=max_px).astype(np.uint8)
    assert np.array_equal(stages.max_scale_lut(b, max_px), want)
    assert want[0] == 0 and want[-1] == max_px  # every b here is at most 65535
