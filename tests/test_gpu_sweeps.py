"""Seeded random sweeps of the kernels added after the original hot path (the intensity passes,
the field warp, the bidirectional-scan phase sums, the exact resize) against their numpy
restatements, and of the two bilinear warps (one, three and four channels, sources and outputs
on and off the 16- and 4-byte grids their vector loads and stores assume) against the C oracle,
and of the normalisation front end (part lists, percentiles) against np.percentile and the
reference's scaling expression, bit for bit: tests/sweep_cases.py draws the cases (shapes, rectangles, tilings,
radii, fields, maps, slab layouts with misaligned starts, index lists with holes) and compares;
tests/test_sweep_cases_host.py holds what the committed seeds reach.  Outputs with an ``out``
argument are written into the middle of a sentinel-filled buffer whose sentinels must survive.
A failure names the kernel, the seed and the drawn parameters; tools/kernel_sweeps.py runs the
same code over any seed range."""
import pytest

import sweep_cases as sc

pytestmark = pytest.mark.gpu


def _seeds(kernel):
    return list(sc.SEEDS[kernel]) + [s for k, s in sc.PINNED if k == kernel]


@pytest.mark.parametrize("seed", _seeds("frame_stats"))
def test_frame_stats_and_stack_sum_sweep(dev, seed):
    sc.check("frame_stats", seed, dev)


@pytest.mark.parametrize("seed", _seeds("shift_search"))
def test_shift_search_sweep(dev, seed):
    sc.check("shift_search", seed, dev)


@pytest.mark.parametrize("seed", _seeds("gradient_sums"))
def test_gradient_sums_sweep(dev, seed):
    sc.check("gradient_sums", seed, dev)


@pytest.mark.parametrize("seed", _seeds("tile_gradient_sums"))
def test_tile_gradient_sums_sweep(dev, seed):
    sc.check("tile_gradient_sums", seed, dev)


@pytest.mark.parametrize("seed", _seeds("phase_sums"))
def test_bidi_phase_sums_sweep(dev, seed):
    sc.check("phase_sums", seed, dev)


@pytest.mark.parametrize("seed", _seeds("warp_field"))
def test_warp_field_sweep(dev, seed):
    sc.check("warp_field", seed, dev)


@pytest.mark.parametrize("seed", _seeds("resize_u8"))
def test_resize_u8_sweep(dev, seed):
    sc.check("resize_u8", seed, dev)


@pytest.mark.parametrize("seed", _seeds("warp_affine"))
def test_warp_affine_sweep(dev, seed):
    sc.check("warp_affine", seed, dev)


@pytest.mark.parametrize("seed", _seeds("warp_perspective"))
def test_warp_perspective_sweep(dev, seed):
    sc.check("warp_perspective", seed, dev)


@pytest.mark.parametrize("seed", _seeds("normalize"))
def test_normalize_sweep(dev, seed):
    """stages.brightest_px over the slabs as a part list == np.percentile, and max_scale_u8 of
    every slab == the reference's expression at that value."""
    sc.check("normalize", seed, dev)
