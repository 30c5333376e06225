"""kcmc_amd._intensity: what the quality metrics, the fallback and the refinement share on the
host -- the sample mask, the runs of frames to warp again (hand-written cases, no GPU) and the
per-slab dispatcher of the two indexed kernels (GPU, bit for bit against the restatements of
tests/test_fallback_host.py and tests/test_refine_host.py)."""
import numpy as np
import pytest
import torch

import test_fallback_host as fhost
import test_refine_host as rhost
from kcmc_amd import _intensity, fallback, refine


def test_sample_mask():
    m = _intensity.sample_mask(10, 3, [3, 12, -1, np.int64(9)])
    assert m.dtype == np.bool_ and m.tolist() == [True, False, False, False, False, False, True, False, False, False]
    assert _intensity.sample_mask(4, 1, []).all()
    assert _intensity.sample_mask(5, 2, [1, 3]).tolist() == [True, False, True, False, True]  # no sample skipped
    assert not _intensity.sample_mask(5, 2, [0, 2, 4]).any()
    assert _intensity.sample_mask(0, 1, []).shape == (0,)


def _pairs(sizes):
    """CPU stand-ins for the (source, aligned) slabs of a stack cut into ``sizes`` frames."""
    sources = [torch.zeros((n, 2, 2), dtype=torch.uint16) for n in sizes]
    parts = [torch.zeros((n, 2, 2), dtype=torch.uint16) for n in sizes]
    return sources, parts


def _runs(sizes, idxs, chunk=None):
    sources, parts = _pairs(sizes)
    got = []
    for src, dst, f0, a, b in _intensity.rewarp_runs(sources, parts, idxs, chunk):
        k = [i for i, p in enumerate(parts) if p is dst]
        assert len(k) == 1 and src is sources[k[0]] and f0 == sum(sizes[:k[0]])
        got.append((k[0], a, b))
    return got


def test_rewarp_runs():
    assert _runs([3, 4], []) == []                                  # nothing selected
    assert _runs([3, 4], [9, -1]) == []                             # ... or nothing inside the stack
    assert _runs([3, 4], [2, 1]) == [(0, 1, 3)]                     # a run that ends at the slab boundary
    assert _runs([3, 4], [2, 3, 4]) == [(0, 2, 3), (1, 0, 2)]       # a set across the boundary: one run per slab
    assert _runs([3, 4], [0, 2, 5, 6, 4]) == [(0, 0, 1), (0, 2, 3), (1, 1, 4)]
    assert _runs([3, 4], {1: "a", 2: "b"}, chunk=1) == [(0, 1, 2), (0, 2, 3)]  # a mapping's keys; one frame a piece
    assert _runs([3, 4], [1, 2], chunk=10) == [(0, 1, 3)]           # a chunk longer than the run
    assert _runs([7], range(7), chunk=3) == [(0, 0, 3), (0, 3, 6), (0, 6, 7)]
    assert _runs([7], [0, 1, 2, 3, 5, 6], chunk=3) == [(0, 0, 3), (0, 3, 4), (0, 5, 7)]  # chunks restart with the run


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["shift_search", "gradient_sums"])
def test_indexed_dispatch_over_slab_views(dev, kernel):
    """Two slabs that are views of one allocation (the second starts off the 16-byte grid), a
    repeated, an unordered and two out-of-range indices: every row is its frame's, whichever
    slab holds it, and the rows of the indices outside the stack are zero."""
    H, W, rect = 33, 41, (4, 29, 5, 36)
    rng = np.random.default_rng(41)
    x = rng.integers(0, 65536, (5, H, W)).astype(np.uint16)
    ref = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    t = torch.from_numpy(x).to(dev)
    slabs = [t[:2], t[2:]]
    assert slabs[0].data_ptr() % 16 == 0 and slabs[1].data_ptr() % 16 == 4 and slabs[1].is_contiguous()
    idx = [4, 0, 4, 7, -1, 2]
    if kernel == "shift_search":
        got = fallback.shift_search(slabs, idx, ref, rect, 2)
        want = fhost.ref_shift_search(x, idx, ref, rect, 2).astype(np.int64)
        assert got.shape == (6, 5, 5, 5)
        np.testing.assert_array_equal(got, want)
    else:
        got = refine.gradient_sums(slabs, idx, ref, rect)
        want = rhost.ref_gradient_sums(x, idx, ref, rect)
        assert got.shape == (6, 7)
        assert [[int(v) for v in r] for r in got] == [[int(v) for v in r] for r in want]
    assert not got[3].any() and not got[4].any() and got[0].any() and got[5].any()
    np.testing.assert_array_equal(got[0], got[2])
