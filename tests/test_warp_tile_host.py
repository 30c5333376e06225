"""Which paths of the shared tile skeleton (csrc/warp_tile.h) the GPU cases of the bicubic warp
(test_gpu_warp_cubic.py) and of the field warp (test_gpu_piecewise.py, the committed warp_field
sweep seeds) reach, worked out on the host: a numpy restatement of the plan (DESIGN.md K3f "Box
bound", K3c "Layout and bound") classifies every tile of every case, and the union must hold
every path.  A break in a path no case reaches would go unseen on the device.  (Today the existing
cases reach them all, so no GPU case had to be added for a path.)"""
import numpy as np

import sweep_cases
import test_gpu_piecewise as gp
import test_gpu_warp_cubic as gc
from test_warp_cubic_host import _invert, rot_about_centre, shift_map

TILE_W, MAX_PITCH, MAX_ROWS, LDS_ELEMS, LIM, MAX_Q = 128, 256, 72, 10240, 30000, 1 << 20


# ------------------------------------------------------------------ the plan, restated
def affine_box(m, xb, yb, xl, yl):
    """Minimum and maximum of X and of Y over the tile in 1/1024 px: the affine part is separable
    and monotone, so they are taken at the corner columns and rows."""
    def r(v):
        assert abs(v) < 2 ** 31 - 16  # the device rounds to int32
        return int(np.rint(v))

    a, b = [r(m[0] * x * 1024) for x in (xb, xl)], [r(m[3] * x * 1024) for x in (xb, xl)]
    x = [r((m[1] * y + m[2]) * 1024) + 16 for y in (yb, yl)]
    y = [r((m[4] * y + m[5]) * 1024) + 16 for y in (yb, yl)]
    return min(x) + min(a), max(x) + max(a), min(y) + min(b), max(y) + max(b)


def classify_box(sx0, sx1, sy0, sy1, H, W, extra_ok=True):
    small = extra_ok and all(-LIM < v < LIM for v in (sx0, sx1, sy0, sy1))
    ax0 = sx0 // 8 * 8
    pitch, rows = (sx1 - ax0 + 1 + 7) // 8 * 8, sy1 - sy0 + 1
    if small and (sx1 < 0 or sx0 > W - 1 or sy1 < 0 or sy0 > H - 1):
        return "zeros"
    if small and pitch <= MAX_PITCH and rows <= MAX_ROWS and pitch * rows <= LDS_ELEMS:
        return "staged-inside" if sx0 >= 0 and sx1 <= W - 1 and sy0 >= 0 and sy1 <= H - 1 else "staged-border"
    return "gather"


def node0(p, L, g):
    """The first of the two nodes that pixel index p mixes along an axis of length L with g nodes."""
    return 0 if g == 1 else min(min(max((2 * p + 1) * g - L, 0), 2 * L * (g - 1)) // (2 * L), g - 2)


def tile_paths(M, H, W, inverse_map, vec, q=None):
    """The paths the tiles of one frame take.  q None: the bicubic warp (box widened by -1 / +2);
    q [gy, gx, 2]: the field warp (box moved by the extrema of the nodes the tile mixes)."""
    m = np.asarray(M, np.float64).reshape(6) if inverse_map else _invert(M)
    tile_h = 64 if H % 64 == 0 and H % 56 != 0 else 56
    paths = {f"tile{tile_h}"}
    for yb in range(0, H, tile_h):
        for xb in range(0, W, TILE_W):
            xl, yl = min(xb + TILE_W, W) - 1, min(yb + tile_h, H) - 1
            if np.isnan(m).any():
                paths.add("nan")
                continue
            x0, x1, y0, y1 = affine_box(m, xb, yb, xl, yl)
            if q is None:
                path = classify_box((x0 >> 10) - 1, (x1 >> 10) + 2, (y0 >> 10) - 1, (y1 >> 10) + 2, H, W)
            else:
                gy, gx = q.shape[:2]
                Q = q[node0(yb, H, gy):min(node0(yl, H, gy) + 1, gy - 1) + 1,
                      node0(xb, W, gx):min(node0(xl, W, gx) + 1, gx - 1) + 1].astype(np.int64)
                ok = bool(np.abs(Q).max() <= MAX_Q)
                (qx0, qy0), (qx1, qy1) = Q.min((0, 1)), Q.max((0, 1))
                path = classify_box((x0 + qx0) >> 10, ((x1 + qx1) >> 10) + 1, (y0 + qy0) >> 10, ((y1 + qy1) >> 10) + 1,
                                    H, W, ok).replace("-inside", "").replace("-border", "")
                path = path if ok else "gather-contract"
            paths.add(path)
            if path.startswith("staged"):
                paths.add("vector" if vec else "element-wise")
    return paths


# ------------------------------------------------------------------ the restatement's own answers
def test_restated_plan_on_known_tiles():
    one = lambda *a, **k: tile_paths(*a, **k) - {"tile56", "tile64"}  # noqa: E731
    assert one(shift_map(0, 0), 56, 128, True, True) == {"staged-border", "vector"}  # taps one column outside
    assert one(shift_map(5, 7), 128, 264, True, True) >= {"staged-inside", "staged-border"}
    assert one(shift_map(300, 0), 56, 128, True, True) == {"zeros"}
    assert one(shift_map(-40000, 0), 56, 128, True, True) == {"gather"}  # beyond the coordinate limit
    assert one(rot_about_centre(np.deg2rad(20), 56, 128), 56, 128, False, False) == {"gather"}  # > 72 rows
    assert one(shift_map(np.nan, 0), 56, 128, True, True) == {"nan"}
    z = np.zeros((3, 3, 2), np.int32)
    assert one(shift_map(0, 0), 56, 129, True, False, z) == {"staged", "element-wise"}
    assert one(shift_map(0, 0), 56, 128, True, True, z + (1 << 20)) == {"zeros"}
    assert one(shift_map(0, 0), 56, 128, True, True, z + (1 << 20) + 1) == {"gather-contract"}
    assert "tile64" in tile_paths(shift_map(0, 0), 128, 8, True, True)
    assert "tile56" in tile_paths(shift_map(0, 0), 448, 8, True, True)  # H % 64 == 0 and H % 56 == 0
    assert [node0(p, 10, 2) for p in range(10)] == [0] * 10 and node0(5, 9, 1) == 0
    # 12 pixels, 4 nodes: centres at 1, 4, 7, 10; held constant outside the outermost two
    assert [node0(p, 12, 4) for p in (0, 1, 3, 4, 6, 7, 10, 11)] == [0, 0, 0, 1, 1, 2, 2, 2]


# ------------------------------------------------------------------ the GPU cases
def cubic_cases():
    """(H, W, map, inverse_map, 16-byte staging loads) of every call the bicubic GPU tests make
    with their own maps: SIZES x both map families, the clamping sizes, the views, the sweep.  A
    tensor of its own is 16-byte aligned; a view one element in is not."""
    nan = shift_map(np.nan, 0)
    for H, W in gc.SIZES + gc.CLAMP_SIZES:
        maps = gc.inverse_maps(H, W) if (H, W) in gc.SIZES else gc.clamp_maps(H, W)
        for _, m in maps + [("nan", nan)]:
            yield H, W, m, True, W % 8 == 0
        for m in gc.with_nan(np.stack([m for _, m in gc.forward_maps(H, W)])):
            yield H, W, m, False, W % 8 == 0
    for H, W in gc.VIEW_SIZES:
        for s_off, _ in gc.VIEW_OFFSETS:
            for _, m in gc.view_maps(H, W):
                yield H, W, m, True, W % 8 == 0 and s_off == 0
    for _, H, W, _, inv, _, maps in gc.sweep_cases():
        for m in maps:
            yield H, W, m, inv, W % 8 == 0


def field_cases():
    """(H, W, map, q [gy, gx, 2], inverse_map, 16-byte staging loads, far field) per frame: CASES
    both ways, the far field of test_constant_field_..., the 16 committed sweep seeds slab by slab."""
    for grid, amp, (F, H, W), _ in gp.CASES:
        q, M = gp.random_field(grid, amp, (F, H, W))
        for f in range(F):
            for inv in (False, True):
                yield H, W, M[f], q[f], inv, W % 8 == 0, False
    F, H, W = gp.FAR_SHAPE
    for qf in gp.far_field():
        yield H, W, shift_map(0, 0), qf, False, W % 8 == 0, True
    for seed in sweep_cases.SEEDS["warp_field"]:
        c = sweep_cases.case_warp_field(seed)
        for a, b, off in c["slabs"]:
            for f in range(a, b):
                yield c["H"], c["W"], c["M"][f], c["q"][f], c["inverse_map"], c["W"] % 8 == 0 and off % 8 == 0, False


CUBIC_PATHS = {"vector", "element-wise", "zeros", "gather", "nan", "tile56", "tile64", "staged-inside", "staged-border"}
FIELD_PATHS = {"vector", "element-wise", "zeros", "gather", "nan", "tile56", "tile64", "staged", "gather-contract"}


def test_the_bicubic_gpu_cases_reach_every_path():
    reached = set()
    for H, W, m, inv, vec in cubic_cases():
        reached |= tile_paths(m, H, W, inv, vec)
    assert reached == CUBIC_PATHS


def test_the_field_gpu_cases_reach_every_path():
    reached, far = set(), set()
    for H, W, m, q, inv, vec, is_far in field_cases():
        p = tile_paths(m, H, W, inv, vec, q)
        reached |= p
        far |= p if is_far else set()
    assert reached == FIELD_PATHS
    assert "gather-contract" in far  # the existing case with nodes outside the contract
