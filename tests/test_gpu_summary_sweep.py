"""Seeded random sweep of kcmc_temporal_sums_u16 against the restatement of
tests/test_summary_host.py, bit for bit, in the style of tests/sweep_cases.py (whose shared
draws it uses): H and W in [1, 48] (about half the widths a multiple of 8), F in [1, 80] (up to
three chunks of frames), a rectangle (one pixel, the whole image, or any), a selection (none,
random, or no frame at all), 4 or 8 neighbours, and the stack cut into 1 to 3 slabs that start
0, 2, 8 or 16 bytes into their allocations.  Every slab goes through the C entry as it is, into
sentinel-guarded outputs, and the slabs' planes are added on the host; the same case goes
through kcmc_amd.summary.temporal_sums.  case(seed) needs no GPU."""
import numpy as np
import pytest

import sweep_cases as sc
import test_summary_host as host

SEEDS = tuple(range(32))


def case(seed):
    # stream 7: the one behind sweep_cases' first seven kernels (once len(sc.KERNELS)); a literal,
    # so that kernels appended there leave these cases as they are (warp_affine now seeds from
    # the same stream, which harms neither)
    rng = np.random.default_rng([7, int(seed)])
    F, H, W = int(rng.integers(1, 81)), int(rng.integers(1, 49)), sc._width(rng, 1, 48)
    c = sc._stack_case(rng, F, H, W, with_ref=False)
    c["rect"] = sc._rect(rng, H, W, 0, int(rng.integers(0, 8)))
    kind = int(rng.integers(0, 8))
    c["sel"] = None if kind < 3 else np.zeros(F, bool) if kind == 3 else rng.random(F) < 0.6
    c["neighbours"] = int(rng.choice([4, 8]))
    return c


def test_cases_reach_the_paths_the_sweep_is_for():
    cases = [case(s) for s in SEEDS]
    vec = [c["W"] % 8 == 0 and all(off % 8 == 0 for _, _, off in c["slabs"]) for c in cases]
    assert 4 <= sum(vec) <= len(cases) - 8                                   # 16-byte and element path
    assert any(c["W"] % 8 == 0 and any(off % 8 for _, _, off in c["slabs"]) for c in cases)  # unaligned base
    assert {c["neighbours"] for c in cases} == {4, 8}
    assert any(c["sel"] is None for c in cases) and any(c["sel"] is not None and c["sel"].any() for c in cases)
    assert any(c["sel"] is not None and not c["sel"].any() for c in cases)
    assert any(b - a > 64 for c in cases for a, b, _ in c["slabs"])           # three chunks in one call
    assert any(len(c["slabs"]) == 3 for c in cases) and any(len(c["slabs"]) == 1 for c in cases)
    assert any(c["H"] > 16 for c in cases) and any(c["H"] * c["W"] % 2 for c in cases)  # two tile rows; odd H * W
    rects = [c["rect"] for c in cases]
    assert any(r[1] - r[0] == 1 and r[3] - r[2] == 1 for r in rects)
    assert any(r[2] % 8 and r[3] % 8 for r in rects)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_temporal_sums_sweep(dev, seed):
    from kcmc_amd import summary
    from test_gpu_summary import entry

    c = case(seed)
    msg = f"seed {seed}: {sc.describe(c)}"
    n, planes, top = host.ref_temporal_sums(c["frames"], c["rect"], c["sel"], c["neighbours"])
    parts = [sc._view(c["frames"][a:b], off, dev) for a, b, off in c["slabs"]]
    got_planes, got_top = np.zeros_like(planes), np.zeros_like(top)
    for p, (a, b, off) in zip(parts, c["slabs"]):
        assert p.data_ptr() % 16 == (2 * off) % 16
        pl, tp = entry(p, c["rect"], None if c["sel"] is None else c["sel"][a:b], c["neighbours"], dev)
        got_planes += pl
        got_top = np.maximum(got_top, tp)
    np.testing.assert_array_equal(got_planes, planes, err_msg=msg)
    np.testing.assert_array_equal(got_top, top, err_msg=msg)
    gn, gp, gt = summary.temporal_sums(parts[0] if len(parts) == 1 else parts, c["rect"], c["sel"], c["neighbours"])
    assert gn == n, msg
    np.testing.assert_array_equal(gp.cpu().numpy(), planes, err_msg=msg)
    np.testing.assert_array_equal(gt.cpu().numpy(), top, err_msg=msg)
